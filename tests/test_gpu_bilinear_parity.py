"""bilinear on the device vs the oracle (oracle/gridpp_oracle.c: orc_bilinear, pinned on the reference's
tests/test_bilinear.py values by tests/test_oracle_golden.py).  The box search and the weights are float / double
expressions in the reference's own association, so the comparison is exact (NaN == NaN); the one tolerance (1e-6 relative)
is there for the double pow(x, 2) of the host libm inside the general-quadrilateral root."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-6


def _regular(Y, X, lat0=50.0, lat1=52.0, lon0=5.0, lon1=8.0):
    return np.meshgrid(np.linspace(lat0, lat1, Y), np.linspace(lon0, lon1, X), indexing="ij")


def _warped(Y, X, seed):
    """A rotated, sheared and mildly curved mesh.  Its cells are 0.02 x 0.015 degrees and the curvature terms 2e-5 / 1e-5, so both
    cross products of every box stay below the weights' absolute 1e-4 (the largest is 3.3e-7): what this mesh tests is the
    parallelogram formula on rotated and sheared boxes.  The general-quadrilateral solve is tested on the meshes of
    tests/bilinear_cases.py (tests/test_gpu_bilinear_general.py)."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(Y, dtype=float), np.arange(X, dtype=float), indexing="ij")
    a = np.deg2rad(rng.uniform(-30, 30))
    u = 0.02 * (i * np.cos(a) - j * np.sin(a)) + 2e-5 * i * j
    v = 0.015 * (i * np.sin(a) + j * np.cos(a)) + 1e-5 * i * i
    return 55 + v, 8 + u


def _all_parallelogram(lats, lons):
    from tests.bilinear_cases import classify
    cl = classify(lats, lons)
    return cl["parallelogram"] == cl["boxes"] > 0


def _field(Y, X, seed, nan_frac=0.0, T=None):
    rng = np.random.default_rng(seed)
    shape = (Y, X) if T is None else (T, Y, X)
    f = rng.normal(0, 3, shape).astype(np.float32)
    if nan_frac:
        f[rng.random(shape) < nan_frac] = np.nan
    return f


def _queries(lats, lons, n, seed, margin=0.1):
    rng = np.random.default_rng(seed)
    dlat, dlon = lats.max() - lats.min(), lons.max() - lons.min()
    qlat = lats.min() - margin * dlat + (1 + 2 * margin) * dlat * rng.random(n)
    qlon = lons.min() - margin * dlon + (1 + 2 * margin) * dlon * rng.random(n)
    k = min(200, lats.size)                      # exact grid nodes, too (s / t land on 0 or 1)
    qlat[:k], qlon[:k] = lats.ravel()[:k], lons.ravel()[:k]
    return qlat, qlon


def _check(out, ref):
    out, ref = np.asarray(out), np.asarray(ref)
    assert out.shape == ref.shape
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    np.testing.assert_allclose(out, ref, rtol=RTOL, atol=1e-6)
    return float(np.mean((out == ref) | (np.isnan(out) & np.isnan(ref))))


@pytest.mark.parametrize("mesh", ["regular", "warped", "cartesian"])
@pytest.mark.parametrize("nan_frac", [0.0, 0.05])
def test_grid_to_points_matches_oracle(mesh, nan_frac):
    import gridpp_amd as gridpp
    from oracle import oracle as O
    Y, X = 61, 83
    ctype = gridpp.Cartesian if mesh == "cartesian" else gridpp.Geodetic
    if mesh == "regular":
        lats, lons = _regular(Y, X)
    elif mesh == "warped":
        lats, lons = _warped(Y, X, 3)
        assert _all_parallelogram(lats, lons)
    else:
        lats, lons = np.meshgrid(np.linspace(0, 60000, Y), np.linspace(-1000, 90000, X), indexing="ij")
    vals = _field(Y, X, 11, nan_frac)
    qlat, qlon = _queries(lats, lons, 6000, 5)
    out = gridpp.bilinear(gridpp.Grid(lats, lons, type=ctype), gridpp.Points(qlat, qlon, type=ctype), vals)
    ref = O.bilinear(O.Pts(lats.ravel(), lons.ravel(), ctype=ctype), (Y, X), O.Pts(qlat, qlon, ctype=ctype), vals)
    exact = _check(out, ref)
    assert exact > 0.999, exact
    near = O.nearest(O.Pts(lats.ravel(), lons.ravel(), ctype=ctype), O.Pts(qlat, qlon, ctype=ctype), vals)
    assert np.mean(ref != near) > 0.3          # the case exercises the interpolation, not only the fallback


def test_time_levels_and_grid_output_match_oracle():
    import gridpp_amd as gridpp
    from oracle import oracle as O
    Y, X, T = 40, 50, 7
    lats, lons = _warped(Y, X, 8)
    assert _all_parallelogram(lats, lons)
    olats, olons = _regular(33, 47, lats.min(), lats.max(), lons.min(), lons.max())
    vals = _field(Y, X, 2, 0.03, T)
    igrid, ogrid = gridpp.Grid(lats, lons), gridpp.Grid(olats, olons)
    out = gridpp.bilinear(igrid, ogrid, vals)
    assert np.shape(out) == (T, 33, 47)
    ref = O.bilinear(O.Pts(lats.ravel(), lons.ravel()), (Y, X), O.Pts(olats.ravel(), olons.ravel()), vals).reshape(T, 33, 47)
    _check(out, ref)
    # every level equals the 2-D call on that level
    for t in (0, T - 1):
        np.testing.assert_array_equal(np.asarray(out)[t], np.asarray(gridpp.bilinear(igrid, ogrid, vals[t])))


def test_device_tensors_in_and_out():
    import torch
    import gridpp_amd as gridpp
    Y, X, T = 64, 64, 3
    lats, lons = _regular(Y, X)
    vals = _field(Y, X, 4, 0.0, T)
    qlat, qlon = _queries(lats, lons, 3000, 9)
    grid, pts = gridpp.Grid(lats, lons), gridpp.Points(qlat, qlon)
    host = gridpp.bilinear(grid, pts, vals)
    dev = gridpp.bilinear(grid, pts, torch.from_numpy(vals).cuda())
    assert dev.is_cuda and tuple(dev.shape) == (T, 3000)
    np.testing.assert_array_equal(dev.cpu().numpy(), host)


def test_get_box_matches_oracle():
    import gridpp_amd as gridpp
    from oracle import oracle as O
    Y, X = 25, 31
    lats, lons = _warped(Y, X, 21)
    assert _all_parallelogram(lats, lons)
    grid = gridpp.Grid(lats, lons)
    og = O.Pts(lats.ravel(), lons.ravel())
    qlat, qlon = _queries(lats, lons, 300, 2)
    for la, lo in zip(qlat, qlon):
        assert grid.get_box(float(np.float32(la)), float(np.float32(lo))) == O.get_box(og, (Y, X), float(np.float32(la)), float(np.float32(lo)))


def test_distorted_box_raises_like_the_reference():
    """bilinear.cpp:309-313: weights outside [0, 1] -> std::runtime_error.  A millidegree-sized box passes both
    "parallel" tests (their tolerance is an absolute 1e-4), so the parallelogram formula is applied to a kite and the
    weights near the far corner come out as 2.5; the oracle rejects the location and so must the device."""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    lats = np.array([[0, -0.002], [0.001, 0.001]])
    lons = np.array([[0, 0.003], [0, 0.001]])
    vals = np.array([[0, 1], [2, 3]], np.float32)
    grid = gridpp.Grid(lats, lons, type=gridpp.Cartesian)
    og = O.Pts(lats.ravel(), lons.ravel(), ctype=1)
    with pytest.raises(O.OracleDistorted):
        O.bilinear(og, (2, 2), O.Pts([-0.0015], [0.0025], ctype=1), vals)
    with pytest.raises(RuntimeError, match="Problem with bilinear interpolation"):
        gridpp.bilinear(grid, gridpp.Points([-0.0015], [0.0025], type=gridpp.Cartesian), vals)
    # a location near the well-behaved corner of the same box is fine
    ok = gridpp.bilinear(grid, gridpp.Points([0.0005], [0.0005], type=gridpp.Cartesian), vals)
    np.testing.assert_array_equal(ok, O.bilinear(og, (2, 2), O.Pts([0.0005], [0.0005], ctype=1), vals))


def test_full_size_properties():
    """Reference benchmark shape (tests/benchmark.py:57-58: 1000x1000 grid -> the same grid, 2-D and x50 levels): a grid
    interpolated onto itself returns the field; a field that is linear in (lon, lat) is reproduced between the nodes."""
    import torch
    import gridpp_amd as gridpp
    N, T = 1000, 50
    lats, lons = np.meshgrid(np.linspace(0, 1, N), np.linspace(0, 1, N), indexing="ij")
    grid = gridpp.Grid(lats, lons)
    vals = torch.randn((T, N, N), device="cuda")
    out = gridpp.bilinear(grid, grid, vals)
    assert tuple(out.shape) == (T, N, N)
    assert torch.allclose(out, vals, rtol=1e-5, atol=1e-5)    # (1 / p) * p may be 1 - ulp: a weight of 0.99999994, not 1
    mid_lats = (lats[:-1, :-1] + lats[1:, 1:]) / 2
    mid_lons = (lons[:-1, :-1] + lons[1:, 1:]) / 2
    lin = (2.0 * lons + 3.0 * lats).astype(np.float32)
    got = gridpp.bilinear(grid, gridpp.Grid(mid_lats, mid_lons), lin)
    np.testing.assert_allclose(got, 2.0 * mid_lons + 3.0 * mid_lats, atol=2e-5)
