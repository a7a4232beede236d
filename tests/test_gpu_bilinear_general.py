"""bilinear and the Bilinear downscalers where every box is a general quadrilateral: k_bilinear (gridpp_amd/csrc/bilinear.hip) and
k_downscale<true> (downscale.hip), both through the direct locator of downscale_loc.h and weights_general of bilinear_geom.h, on the
cases of tests/bilinear_cases.py.
tests/test_bilinear_cases_oracle.py asserts on the CPU that those cases take all three branches and both roots of the solve and
that the oracle agrees with a float64 Newton inversion; here the device is compared with the oracle (a few float32 ulps of the
largest value, almost all outputs bit-identical), with the Newton inversion itself, and with the oracle's box search.

The bound against the oracle, 4 * 2^-23 * max|values|: the two sides may differ by one ulp of a double root (sqrt, or pow(x, 2)
against x * x), which can move s or t by one float32 ulp (at most 2^-23); the value is a convex combination of corners bounded by
max|values|, formed in four float products and three sums."""
import ctypes as C

import numpy as np
import pytest

from tests import bilinear_cases as B
from tests.test_bilinear_cases_oracle import REFERENCE_THROWS, VALUE_CASES

pytestmark = pytest.mark.gpu
F32 = np.float32
ULPS = 4 * 2.0 ** -23
DISTORTED = "Problem with bilinear interpolation"


def _grid(c):
    import gridpp_amd as gridpp
    return gridpp.Grid(c.lats, c.lons, type=c.ctype)


def _points(c, n=None):
    import gridpp_amd as gridpp
    return gridpp.Points(c.qlat[:n], c.qlon[:n], type=c.ctype)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _check(out, ref, vmax):
    """identical NaN pattern, |out - ref| <= 4 * 2^-23 * vmax -> the share of bit-identical outputs"""
    out, ref = np.asarray(out), np.asarray(ref)
    assert out.shape == ref.shape and out.dtype == F32
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    fin = np.isfinite(ref)
    assert np.array_equal(out[~fin], ref[~fin], equal_nan=True)
    err = np.abs(out[fin].astype(np.float64) - ref[fin].astype(np.float64))
    assert err.size == 0 or float(err.max()) <= ULPS * vmax, (float(err.max()), ULPS * vmax)
    return float(np.mean(_same(out, ref)))


# ---- values ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", VALUE_CASES)
def test_matches_oracle(cid):
    import gridpp_amd as gridpp
    c = B.case(cid)
    out = gridpp.bilinear(_grid(c), _points(c), c.values)
    exact = _check(out, c.oracle_values, float(np.abs(c.values).max()))
    print("%s: %.5f of %d outputs bit-identical to the oracle" % (cid, exact, out.size))
    assert exact >= 0.99, exact


@pytest.mark.parametrize("cid", VALUE_CASES)
def test_against_float64_newton(cid):
    """the kernel against the reference side, never against itself: e_device <= 2 e_oracle + 4 * 2^-23 * max|values|, for the
    random field and for a field linear in (lon, lat), which every bilinear patch reproduces"""
    import gridpp_amd as gridpp
    c = B.case(cid)
    m = c.boxes[:, 0] != 0
    grid, pts = _grid(c), _points(c)
    for name, field, ref, truth in (("N(0, 3)", c.values, c.oracle_values, c.truth_values[0]), ("linear", c.linear, c.oracle_linear, c.truth_linear)):
        out = gridpp.bilinear(grid, pts, field)
        e_device = float(np.max(np.abs(out[m].astype(np.float64) - truth[m])))
        e_oracle = float(np.max(np.abs(ref[m].astype(np.float64) - truth[m])))
        print("%s %s: e_device = %.3g, e_oracle = %.3g" % (cid, name, e_device, e_oracle))
        assert e_device <= 2 * e_oracle + ULPS * float(np.abs(field).max())
        np.testing.assert_array_equal(out[~m], ref[~m])      # no box: the nearest node, exactly


# ---- boxes ---------------------------------------------------------------------------------------------------------------------------------
def _device_boxes(grid, qlat, qlon):
    """Grid::get_box for many lookups through the batched C entry -> (n, 5) = inside, Y1, X1, Y2, X2"""
    from gridpp_amd import _capi
    qlat, qlon = np.ascontiguousarray(qlat, F32), np.ascontiguousarray(qlon, F32)
    n = qlat.size
    inside, boxes = np.full(n, -7, np.int32), np.full((n, 4), -7, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    _capi.check(_capi.lib().gpp_grid_get_box(grid._h, p(qlat), p(qlon), n, p(inside), p(boxes)))
    return np.concatenate([inside[:, None], boxes], axis=1)


@pytest.mark.parametrize("cid", B.CASE_IDS)
def test_boxes_match_oracle(cid):
    c = B.case(cid)
    got = _device_boxes(_grid(c), c.qlat, c.qlon)
    np.testing.assert_array_equal(got, c.boxes)
    assert 0.5 < np.mean(got[:, 0]) < 0.8      # inside and outside, first and last cell row and column among them
    inside = got[got[:, 0] != 0]
    for k, n in ((1, c.shape[0]), (2, c.shape[1])):
        assert inside[:, k].min() == 0 and inside[:, k].max() == n - 2


# ---- time levels ---------------------------------------------------------------------------------------------------------------------------
def _levels(c):
    """T = 4, another pattern of missing values per level: 0 has a missing corner in at least 10 % of the boxes (the weights of
    those locations are solved at the first later level with four valid corners), 1 is all-valid, 2 and 3 mix NaN and +-inf"""
    rng = np.random.default_rng(300 + B.CASE_IDS.index(c.id))
    v = rng.normal(0, 3, (4,) + c.shape).astype(F32)
    v[0][rng.random(c.shape) < 0.05] = np.nan
    v[2][rng.random(c.shape) < 0.03] = np.inf
    v[2][rng.random(c.shape) < 0.03] = np.nan
    v[3][rng.random(c.shape) < 0.04] = -np.inf
    v[3][rng.random(c.shape) < 0.02] = np.inf
    bad = ~np.isfinite(v[0])
    box_bad = bad[:-1, :-1] | bad[1:, :-1] | bad[:-1, 1:] | bad[1:, 1:]
    assert box_bad.mean() >= 0.10 and np.isfinite(v[1]).all()
    return v


@pytest.mark.parametrize("cid", VALUE_CASES)
def test_time_levels(cid):
    import torch
    import gridpp_amd as gridpp
    c = B.case(cid)
    v = _levels(c)
    grid, pts = _grid(c), _points(c)
    out = gridpp.bilinear(grid, pts, v)
    assert out.shape == (4, B.NQ)
    fin = np.where(np.isfinite(v), v, 0)
    _check(out, c.oracle(v), float(np.abs(fin).max()))
    dev = gridpp.bilinear(grid, pts, torch.from_numpy(v).cuda())
    assert dev.is_cuda and tuple(dev.shape) == (4, B.NQ)
    dev = dev.cpu().numpy()
    for t in range(4):
        level = gridpp.bilinear(grid, pts, v[t])
        assert _same(out[t], level).all() and _same(dev[t], level).all(), t
        level_dev = gridpp.bilinear(grid, pts, torch.from_numpy(v[t]).cuda()).cpu().numpy()
        assert _same(level_dev, level).all(), t
    # level 0 falls back to the nearest node where a corner is missing; the same locations interpolate at level 1
    m = c.boxes[:, 0] != 0
    near0 = gridpp.nearest(grid, pts, v[0])
    lazy = m & _same(out[0], near0) & (out[1] != gridpp.nearest(grid, pts, v[1]))
    assert lazy.sum() > 100


# ---- query counts around the 256-thread block ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["metres_6e5-flipX", "trapezoid0-asis"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_query_counts(cid, n):
    import gridpp_amd as gridpp
    c = B.case(cid)
    # the tail of the list (uniform over the bounding box) and the head (nodes, edge midpoints)
    for sl in (slice(0, n), slice(B.NQ - n, B.NQ)):
        pts = gridpp.Points(c.qlat[sl], c.qlon[sl], type=c.ctype)
        out = gridpp.bilinear(_grid(c), pts, c.values)
        assert out.shape == (n,)
        _check(out, c.oracle_values[sl], float(np.abs(c.values).max()))
        np.testing.assert_array_equal(_device_boxes(_grid(c), c.qlat[sl], c.qlon[sl]), c.boxes[sl])


# ---- grids of height or width 1 or 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", B.DEGENERATE_SHAPES)
def test_degenerate_shapes(shape):
    import gridpp_amd as gridpp
    d = B.degenerate(shape)
    grid = gridpp.Grid(d["lats"], d["lons"], type=gridpp.Cartesian)
    out = gridpp.bilinear(grid, gridpp.Points(d["qlat"], d["qlon"], type=gridpp.Cartesian), d["values"])
    np.testing.assert_array_equal(out, d["expected"])
    np.testing.assert_array_equal(_device_boxes(grid, d["qlat"], d["qlon"]), d["boxes"])
    out3 = gridpp.bilinear(grid, gridpp.Points(d["qlat"], d["qlon"], type=gridpp.Cartesian), np.stack([d["values"], -d["values"]]))
    np.testing.assert_array_equal(out3, np.stack([d["expected"], -d["expected"]]))


# ---- where the reference throws -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", REFERENCE_THROWS)
def test_general_box_without_a_second_root_raises_like_the_reference(cid):
    """qa == 0 with the first root out of range (tests/test_bilinear_cases_oracle.py: REFERENCE_THROWS): the oracle raises for every
    location inside the mesh, and so must bilinear and the Bilinear downscalers; a location with no box is the nearest node"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = B.case(cid)
    grid = _grid(c)
    m = c.boxes[:, 0] != 0
    with pytest.raises(O.OracleDistorted):
        c.oracle(c.values)
    with pytest.raises(RuntimeError, match=DISTORTED):
        gridpp.bilinear(grid, _points(c), c.values)
    i = int(np.nonzero(m)[0][-1])
    with pytest.raises(O.OracleDistorted):
        O.bilinear(c.opts[0], c.shape, O.Pts(c.qlat[i:i + 1], c.qlon[i:i + 1], ctype=c.ctype), c.values)
    with pytest.raises(RuntimeError, match=DISTORTED):
        gridpp.bilinear(grid, gridpp.Points(c.qlat[i:i + 1], c.qlon[i:i + 1], type=c.ctype), c.values)
    for f in (lambda p: gridpp.downscaling(grid, p, c.values, gridpp.Bilinear), lambda p: gridpp.full_gradient(grid, p, c.values, [], [], gridpp.Bilinear)):
        with pytest.raises(RuntimeError, match=DISTORTED):
            f(_points(c))
    outside = gridpp.Points(c.qlat[~m], c.qlon[~m], type=c.ctype)
    np.testing.assert_array_equal(gridpp.bilinear(grid, outside, c.values), c.nearest[~m])
    np.testing.assert_array_equal(gridpp.downscaling(grid, outside, c.values, gridpp.Bilinear), c.nearest[~m])


# ---- the downscalers ---------------------------------------------------------------------------------------------------------------------
DOWNSCALER_CASES = ["metres_6e5-flipY", "degrees-asis"] + [c for c in B.CASE_IDS if c.startswith("trapezoid")]


@pytest.mark.parametrize("cid", DOWNSCALER_CASES)
def test_downscalers(cid):
    """simple_gradient / full_gradient with the Bilinear downscaler as tests/test_gpu_downscaling_parity.py calls and bounds them
    (test_bilinear_matches_both_compositions); the mesh is the only new thing"""
    import gridpp_amd as gridpp
    from tests.test_gpu_downscaling_parity import Case, close, same_bits
    b = B.case(cid)
    T = None if cid.endswith("asis") else 3
    c = Case((b.lats, b.lons), "points", T, seed=400 + B.CASE_IDS.index(cid), ctype=b.ctype)
    if cid in REFERENCE_THROWS:
        with pytest.raises(RuntimeError, match=DISTORTED):
            gridpp.full_gradient(c.igrid, c.out, c.values, c.egrad, c.lgrad, gridpp.Bilinear)
        with pytest.raises(RuntimeError, match=DISTORTED):
            gridpp.simple_gradient(c.igrid, c.out, c.values, 0.0123, gridpp.Bilinear)
        return
    fused = gridpp.full_gradient(c.igrid, c.out, c.values, c.egrad, c.lgrad, gridpp.Bilinear)
    same_bits(fused, c.full(c.d_device(1)))
    exact = close(fused, c.full(c.d_oracle(1)), c.bound())
    print("%s: %.5f of the finite full_gradient outputs bit-identical to the oracle composition" % (cid, exact))
    assert exact > 0.99
    simple = gridpp.simple_gradient(c.igrid, c.out, c.values, 0.0123, gridpp.Bilinear)
    same_bits(simple, c.simple(c.d_device(1), 0.0123))
    close(simple, c.simple(c.d_oracle(1), 0.0123), c.bound(egrad=False, lgrad=False) + 4e-6 * 0.0123 * (3000 + np.zeros(c.shape)))
    d_near, d_bil = c.d_oracle(0), c.d_oracle(1)
    assert np.mean(d_bil(c.values) != d_near(c.values)) > 0.3
    assert np.mean(d_bil(c.ielevs) != d_near(c.ielevs)) > 0.3
