"""simple_gradient / full_gradient / downscaling on the device (k_downscale, gridpp_amd/csrc/downscale.hip) against the
float32 composition of tests/downscaling_ref.py: every field downscaled on its own, then combined.

Nearest is bit-exact against the composition built on the oracle.  Bilinear is bit-exact against the composition built on
the library's own bilinear / nearest (the fused kernel runs the same d(f), downscale_loc.h), and against the oracle within
a bound that scales with the magnitudes involved: the 1e-6 relative tolerance of test_gpu_bilinear_parity.py applies
to each interpolated field, and a difference of elevations carries it as an absolute error."""
import numpy as np
import pytest

from tests import downscaling_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32


# ---- known answers (tests/golden/downscaling_known_answers.json), all four overload shapes ----------------------------------
def _set(gridpp, d):
    lats, lons, elevs, lafs = R.set_arrays(d)
    if d.get("type", "grid") == "grid":
        return gridpp.Grid(lats, lons, elevs if elevs is not None else ((),), lafs if lafs is not None else ((),))
    return gridpp.Points(lats, lons, elevs if elevs is not None else (), lafs if lafs is not None else ())


KNOWN = [c for c in R.known_answers() if "expected" in c]


@pytest.mark.parametrize("case", KNOWN, ids=[c["id"] for c in KNOWN])
def test_known_answer(case):
    import gridpp_amd as gridpp
    igrid, out = _set(gridpp, case["igrid"]), _set(gridpp, case["output"])
    values = np.asarray(case["values"])
    if case["function"] == "downscaling":
        got = gridpp.downscaling(igrid, out, values, case["downscaler"])
    elif case["function"] == "simple_gradient":
        got = gridpp.simple_gradient(igrid, out, values, case["elev_gradient"], case["downscaler"])
    else:
        got = gridpp.full_gradient(igrid, out, values, np.asarray(case["elev_gradient"]), np.asarray(case["laf_gradient"]), case["downscaler"])
    expected = np.asarray(case["expected"], np.float64)
    assert np.shape(got) == expected.shape
    if case["exact"]:
        np.testing.assert_array_equal(got, expected)
    else:
        np.testing.assert_array_almost_equal(got, expected)


def test_known_answer_shapes_cover_all_four_overloads():
    shapes = {(c["function"], c["output"]["type"], np.ndim(c["values"])) for c in KNOWN}
    for f in ("simple_gradient", "full_gradient", "downscaling"):
        assert {(f, o, n) for o in ("grid", "points") for n in (2, 3)} <= shapes, f


# ---- randomised cases against the composition ---------------------------------------------------------------------------------
def _mesh(kind, Y, X):
    if kind == "regular":
        return np.meshgrid(np.linspace(50.0, 52.0, Y), np.linspace(5.0, 8.0, X), indexing="ij")
    if kind == "warped":   # rotated, sheared, mildly curved: the parallelogram formula on rotated and sheared boxes (see below)
        j, i = np.meshgrid(np.arange(Y, dtype=float), np.arange(X, dtype=float), indexing="ij")
        a = np.deg2rad(17.0)
        return 55 + 0.015 * (i * np.sin(a) + j * np.cos(a)) + 1e-5 * i * i, 8 + 0.02 * (i * np.cos(a) - j * np.sin(a)) + 2e-5 * i * j
    return np.meshgrid(np.linspace(0, 60000, Y), np.linspace(-1000, 90000, X), indexing="ij")


def _spoil(rng, a, frac=0.03, inf=True):
    a = a.astype(F32)
    a[rng.random(a.shape) < frac] = np.nan
    if inf:
        a[rng.random(a.shape) < frac / 3] = np.inf
        a[rng.random(a.shape) < frac / 3] = -np.inf
    return a


class Case:
    def __init__(self, mesh, out_kind, T, seed, Y=41, X=53, ctype=None):
        import gridpp_amd as gridpp
        rng = np.random.default_rng(seed)
        if isinstance(mesh, str):
            self.ctype = gridpp.Cartesian if mesh == "cartesian" else gridpp.Geodetic
            self.lats, self.lons = _mesh(mesh, Y, X)
        else:   # the mesh itself: (lats, lons) arrays and the coordinate type (tests/test_gpu_bilinear_general.py)
            self.ctype = gridpp.Geodetic if ctype is None else ctype
            self.lats, self.lons = (np.asarray(a) for a in mesh)
            Y, X = self.lats.shape
        self.ielevs = _spoil(rng, rng.uniform(0, 1500, (Y, X)), 0.02, False)
        self.ilafs = _spoil(rng, rng.uniform(0, 1, (Y, X)), 0.02, False)
        lead = (T,) if T else ()
        self.values = _spoil(rng, rng.normal(5, 3, lead + (Y, X)))
        self.egrad = _spoil(rng, rng.normal(-0.0065, 0.002, lead + (Y, X)))
        self.lgrad = _spoil(rng, rng.normal(2, 1, lead + (Y, X)))
        la, lo = self.lats, self.lons
        dla, dlo = la.max() - la.min(), lo.max() - lo.min()
        if out_kind == "grid":
            self.qlats, self.qlons = np.meshgrid(np.linspace(la.min() - 0.05 * dla, la.max() + 0.05 * dla, 37),
                                                 np.linspace(lo.min() - 0.05 * dlo, lo.max() + 0.05 * dlo, 43), indexing="ij")
        else:
            n = 3000
            self.qlats = la.min() - 0.08 * dla + 1.16 * dla * rng.random(n)
            self.qlons = lo.min() - 0.08 * dlo + 1.16 * dlo * rng.random(n)
            self.qlats[:150], self.qlons[:150] = la.ravel()[:150], lo.ravel()[:150]   # grid nodes: s / t land on 0 or 1
        self.oelevs = _spoil(rng, rng.uniform(0, 1500, self.qlats.shape))
        self.olafs = _spoil(rng, rng.uniform(0, 1, self.qlats.shape))
        self.igrid = gridpp.Grid(self.lats, self.lons, self.ielevs, self.ilafs, type=self.ctype)
        if out_kind == "grid":
            self.out = gridpp.Grid(self.qlats, self.qlons, self.oelevs, self.olafs, type=self.ctype)
        else:
            self.out = gridpp.Points(self.qlats, self.qlons, self.oelevs, self.olafs, type=self.ctype)
        self.shape = lead + np.shape(self.qlats)

    def d_oracle(self, downscaler):
        from oracle import oracle as O
        return R.oracle_downscaler(O, self.lats, self.lons, self.qlats, self.qlons, downscaler, self.ctype)

    def d_device(self, downscaler):
        import gridpp_amd as gridpp
        return R.device_downscaler(gridpp, self.igrid, self.out, downscaler)

    def full(self, d, egrad=True, lgrad=True):
        return R.compose_full(d, self.values, self.egrad if egrad else None, self.lgrad if lgrad else None, self.ielevs, self.ilafs,
                              self.oelevs, self.olafs).reshape(self.shape)

    def simple(self, d, g):
        return R.compose_simple(d, self.values, self.ielevs, self.oelevs, g).reshape(self.shape)

    def bound(self, egrad=True, lgrad=True):
        """|fused - oracle| allowed for Bilinear full_gradient: 4e-6 of every magnitude the result is formed from"""
        d = self.d_oracle(1)
        a = lambda f: np.abs(np.nan_to_num(d(f), nan=0, posinf=0, neginf=0)).astype(np.float64)   # noqa: E731
        oe = np.abs(np.nan_to_num(self.oelevs, nan=0, posinf=0, neginf=0)).ravel()
        ol = np.abs(np.nan_to_num(self.olafs, nan=0, posinf=0, neginf=0)).ravel()
        b = 1 + a(self.values)
        if egrad:
            b = b + a(self.egrad) * (1 + oe + a(self.ielevs))
        if lgrad:
            b = b + a(self.lgrad) * (1 + ol + a(self.ilafs))
        return (4e-6 * b).reshape(self.shape)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) or np.array_equal(a, b, equal_nan=True), \
        int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b)))))
    # (NaN payloads may differ between the two paths; every other value is the same float)


def close(out, ref, bound):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    assert np.array_equal(np.isinf(out) & (out > 0), np.isinf(ref) & (ref > 0))
    assert np.array_equal(np.isinf(out) & (out < 0), np.isinf(ref) & (ref < 0))
    fin = np.isfinite(ref)
    err = np.abs(out[fin] - ref[fin])
    assert np.all(err <= bound[fin]), float(np.max(err / bound[fin]))
    return float(np.mean(out[fin] == ref[fin]))


MESHES = ["regular", "warped", "cartesian"]


@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("out_kind", ["grid", "points"])
@pytest.mark.parametrize("T", [None, 1, 7])   # None: 2-D values
def test_nearest_is_bit_exact_against_oracle_composition(mesh, out_kind, T):
    import gridpp_amd as gridpp
    c = Case(mesh, out_kind, T, seed=100 + (T or 0))
    d = c.d_oracle(0)
    same_bits(gridpp.full_gradient(c.igrid, c.out, c.values, c.egrad, c.lgrad, gridpp.Nearest), c.full(d))
    same_bits(gridpp.simple_gradient(c.igrid, c.out, c.values, -0.0065, gridpp.Nearest), c.simple(d, -0.0065))
    same_bits(gridpp.downscaling(c.igrid, c.out, c.values, gridpp.Nearest), d(c.values).reshape(c.shape))


@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("out_kind", ["grid", "points"])
@pytest.mark.parametrize("T", [None, 1, 7])
def test_bilinear_matches_both_compositions(mesh, out_kind, T):
    import gridpp_amd as gridpp
    c = Case(mesh, out_kind, T, seed=200 + (T or 0))
    if mesh == "warped":   # millidegree cells: every box passes the weights' absolute 1e-4 and takes the parallelogram formula
        from tests.bilinear_cases import classify
        cl = classify(c.lats, c.lons)
        assert cl["parallelogram"] == cl["boxes"] > 0
    fused = gridpp.full_gradient(c.igrid, c.out, c.values, c.egrad, c.lgrad, gridpp.Bilinear)
    same_bits(fused, c.full(c.d_device(1)))
    ref = c.full(c.d_oracle(1))
    assert close(fused, ref, c.bound()) > 0.99
    simple = gridpp.simple_gradient(c.igrid, c.out, c.values, 0.0123, gridpp.Bilinear)
    same_bits(simple, c.simple(c.d_device(1), 0.0123))
    close(simple, c.simple(c.d_oracle(1), 0.0123), c.bound(egrad=False, lgrad=False) + 4e-6 * 0.0123 * (3000 + np.zeros(c.shape)))
    # the case exercises the interpolation, not only the nearest-neighbour fallback
    d_near, d_bil = c.d_oracle(0), c.d_oracle(1)
    assert np.mean(d_bil(c.values) != d_near(c.values)) > 0.3
    assert np.mean(d_bil(c.ielevs) != d_near(c.ielevs)) > 0.3


def test_missing_data():
    import gridpp_amd as gridpp
    c = Case("warped", "points", 3, seed=7)
    # a grid without elevations: simple_gradient gives NaN everywhere, full_gradient has no elevation term
    bare = gridpp.Grid(c.lats, c.lons, ((),), c.ilafs)
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        assert np.all(np.isnan(gridpp.simple_gradient(bare, c.out, c.values, 0.0, ds)))
        with_term = gridpp.full_gradient(bare, c.out, c.values, c.egrad, c.lgrad, ds)
        without = gridpp.full_gradient(bare, c.out, c.values, [], c.lgrad, ds)
        same_bits(with_term, without)
    # points without lafs: the laf term is 0
    nolaf = gridpp.Points(c.qlats, c.qlons, c.oelevs, type=c.ctype)
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        same_bits(gridpp.full_gradient(c.igrid, nolaf, c.values, c.egrad, c.lgrad, ds),
                  gridpp.full_gradient(c.igrid, nolaf, c.values, c.egrad, np.zeros((0, 0, 0)), ds))
        # one gradient absent, both absent -- against the composition
        d = c.d_device(ds)
        same_bits(gridpp.full_gradient(c.igrid, c.out, c.values, [], c.lgrad, ds), c.full(d, egrad=False))
        same_bits(gridpp.full_gradient(c.igrid, c.out, c.values, c.egrad, [], ds), c.full(d, lgrad=False))
        both = gridpp.full_gradient(c.igrid, c.out, c.values, [], [], ds)
        same_bits(both, c.full(d, False, False))
        same_bits(both, np.asarray(gridpp.downscaling(c.igrid, c.out, c.values, ds)) + F32(0))
    # an empty input grid gives all NaN
    out = gridpp.full_gradient(gridpp.Grid(), c.out, np.zeros((3, 0, 0)), [], [], gridpp.Bilinear)
    assert out.shape == (3, c.qlats.size) and np.all(np.isnan(out))


def test_empty_input_grid_and_no_levels():
    """what the entries do before any kernel of theirs runs: a 0 x 0 input grid gives all NaN (nearest.cpp:132-134,
    bilinear.cpp:37-39: every sum with a missing value is missing), no levels give an empty array"""
    import gridpp_amd as gridpp
    rng = np.random.default_rng(12)
    five = gridpp.Points(50 + rng.random(5), 5 + rng.random(5), rng.uniform(0, 800, 5), rng.random(5))
    seven = gridpp.Points(50 + 2 * rng.random(7), 5 + 3 * rng.random(7), rng.uniform(0, 800, 7), rng.random(7))
    lats, lons = _mesh("regular", 3, 4)
    grid = gridpp.Grid(lats, lons, rng.uniform(0, 800, (3, 4)), rng.random((3, 4)))
    empty, none = np.zeros((3, 0, 0), F32), np.zeros((0, 3, 4), F32)
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        for out in (gridpp.simple_gradient(gridpp.Grid(), five, empty, -0.0065, ds), gridpp.full_gradient(gridpp.Grid(), five, empty, empty, empty, ds),
                    gridpp.downscaling(gridpp.Grid(), five, empty, ds)):
            assert out.shape == (3, 5) and out.dtype == F32 and np.all(np.isnan(out))
        for out in (gridpp.simple_gradient(grid, seven, none, -0.0065, ds), gridpp.full_gradient(grid, seven, none, none, none, ds),
                    gridpp.full_gradient(grid, seven, none, [], [], ds), gridpp.downscaling(grid, seven, none, ds)):
            assert out.shape == (0, 7) and out.dtype == F32


def test_null_output_is_an_argument_error_at_the_c_entries():
    """the shared call shell refuses a NULL `out` before anything is launched, for the direct entries as for those of a plan"""
    import gridpp_amd as gridpp
    from gridpp_amd import _capi
    lib = _capi.lib()
    lats, lons = _mesh("regular", 3, 4)
    grid = gridpp.Grid(lats, lons, np.ones((3, 4)), np.ones((3, 4)))
    pts = gridpp.Points([50.5, 51.0], [5.5, 7.0], [1, 2], [0.5, 0.5])
    v = np.ones((1, 3, 4), F32)
    calls = [lambda: lib.gpp_bilinear(grid._h, pts._h, v.ctypes.data, 1, None, _capi.MEM_HOST)]
    for ds in (0, 1):
        calls.append(lambda ds=ds: lib.gpp_simple_gradient(grid._h, pts._h, v.ctypes.data, 1, -0.0065, ds, None, _capi.MEM_HOST))
        calls.append(lambda ds=ds: lib.gpp_full_gradient(grid._h, pts._h, v.ctypes.data, 1, None, None, ds, None, _capi.MEM_HOST))
    for call in calls:
        assert call() == _capi.GPP_EINVAL
        assert lib.gpp_last_error().decode() == "out is NULL"


def test_distorted_box_raises_where_bilinear_raises():
    """a millidegree kite passes both 'parallel' tests of the weights (tests/test_gpu_bilinear_parity.py); the location near the
    far corner is rejected by bilinear, the one near the well-behaved corner is not"""
    import gridpp_amd as gridpp
    lats = np.array([[0, -0.002], [0.001, 0.001]])
    lons = np.array([[0, 0.003], [0, 0.001]])
    grid = gridpp.Grid(lats, lons, np.array([[1, 2], [3, 4]]), np.array([[0.1, 0.2], [0.3, 0.4]]), type=gridpp.Cartesian)
    bad = gridpp.Points([-0.0015], [0.0025], [10], [0.5], type=gridpp.Cartesian)
    good = gridpp.Points([0.0005], [0.0005], [10], [0.5], type=gridpp.Cartesian)
    vals = np.array([[0, 1], [2, 3]], F32)
    nan = np.full((2, 2), np.nan, F32)
    with pytest.raises(RuntimeError, match="Problem with bilinear interpolation"):
        gridpp.bilinear(grid, bad, vals)
    for f in (lambda p, v: gridpp.full_gradient(grid, p, v, vals, vals, gridpp.Bilinear), lambda p, v: gridpp.simple_gradient(grid, p, v, 1.0, gridpp.Bilinear),
              lambda p, v: gridpp.full_gradient(grid, p, v, vals, [], gridpp.Bilinear), lambda p, v: gridpp.downscaling(grid, p, v, gridpp.Bilinear)):
        with pytest.raises(RuntimeError, match="Problem with bilinear interpolation"):
            f(bad, vals)
        f(good, vals)
    # values with a missing corner: the gradients / elevations / lafs still reach the weights, as in the reference
    with pytest.raises(RuntimeError, match="Problem with bilinear interpolation"):
        gridpp.full_gradient(grid, bad, nan, vals, [], gridpp.Bilinear)
    with pytest.raises(RuntimeError, match="Problem with bilinear interpolation"):
        gridpp.simple_gradient(grid, bad, nan, 1.0, gridpp.Bilinear)
    # no field the reference downscales has four valid corners: no weights, no error (all nearest)
    bare = gridpp.Grid(lats, lons, type=gridpp.Cartesian)
    out = gridpp.full_gradient(bare, bad, nan, [], [], gridpp.Bilinear)
    assert np.all(np.isnan(out))
    out = gridpp.full_gradient(bare, bad, vals, [], [], gridpp.Nearest)
    assert np.all(np.isfinite(out))


def test_device_tensors_and_float64_inputs():
    import torch
    import gridpp_amd as gridpp
    c = Case("warped", "grid", 4, seed=9)
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        host = gridpp.full_gradient(c.igrid, c.out, c.values, c.egrad, c.lgrad, ds)
        dev = gridpp.full_gradient(c.igrid, c.out, *(torch.from_numpy(a).cuda() for a in (c.values, c.egrad, c.lgrad)), ds)
        assert dev.is_cuda and tuple(dev.shape) == host.shape
        same_bits(dev.cpu().numpy(), host)
        hs = gridpp.simple_gradient(c.igrid, c.out, c.values, 0.5, ds)
        same_bits(gridpp.simple_gradient(c.igrid, c.out, torch.from_numpy(c.values).cuda(), 0.5, ds).cpu().numpy(), hs)
    # mixing host and device field arguments
    with pytest.raises(ValueError):
        gridpp.full_gradient(c.igrid, c.out, torch.from_numpy(c.values).cuda(), c.egrad, c.lgrad, gridpp.Bilinear)
    with pytest.raises(ValueError):
        gridpp.full_gradient(c.igrid, c.out, c.values, torch.from_numpy(c.egrad).cuda(), c.lgrad, gridpp.Bilinear)
    # float64 numpy inputs of >= 1 Mi elements are cast on the device: the same result as float32-cast inputs
    rng = np.random.default_rng(3)
    Y, X, T = 256, 512, 8
    lats, lons = _mesh("regular", Y, X)
    g = gridpp.Grid(lats, lons, rng.uniform(0, 800, (Y, X)), rng.uniform(0, 1, (Y, X)))
    o = gridpp.Points(50 + 2 * rng.random(5000), 5 + 3 * rng.random(5000), rng.uniform(0, 800, 5000), rng.uniform(0, 1, 5000))
    v, e, l_ = rng.normal(0, 3, (T, Y, X)), rng.normal(-0.006, 0.001, (T, Y, X)), rng.normal(1, 1, (T, Y, X))
    assert v.size >= 1 << 20 and v.dtype == np.float64
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        same_bits(gridpp.full_gradient(g, o, v, e, l_, ds), gridpp.full_gradient(g, o, v.astype(F32), e.astype(F32), l_.astype(F32), ds))
        same_bits(gridpp.simple_gradient(g, o, v, 0.25, ds), gridpp.simple_gradient(g, o, v.astype(F32), 0.25, ds))


def test_chain_calc_gradient_full_gradient_optimal_interpolation():
    """a script written for the reference: calc_gradient -> full_gradient(..., gridpp.Bilinear) -> optimal_interpolation"""
    import gridpp
    rng = np.random.default_rng(11)
    Y, X = 60, 70
    ilats, ilons = np.meshgrid(np.linspace(59, 61, Y), np.linspace(9, 12, X), indexing="ij")
    ielevs = (400 + 300 * np.sin(ilats * 3) * np.cos(ilons * 2)).astype(F32)
    ilafs = np.clip(0.5 + 0.5 * np.sin(ilons * 5), 0, 1).astype(F32)
    temp = (10 - 0.0065 * ielevs + rng.normal(0, 0.3, (Y, X))).astype(F32)
    egrad = gridpp.calc_gradient(ielevs, temp, gridpp.LinearRegression, 3, 5, 30, 0)
    lgrad = gridpp.calc_gradient(ilafs, temp, gridpp.LinearRegression, 3, 5, 0.1, 0)
    igrid = gridpp.Grid(ilats, ilons, ielevs, ilafs)
    olats, olons = np.meshgrid(np.linspace(59.1, 60.9, 150), np.linspace(9.1, 11.9, 170), indexing="ij")
    oelevs = (400 + 300 * np.sin(olats * 3) * np.cos(olons * 2) + rng.normal(0, 50, olats.shape)).astype(F32)
    olafs = np.clip(0.5 + 0.5 * np.sin(olons * 5) + rng.normal(0, 0.1, olats.shape), 0, 1).astype(F32)
    ogrid = gridpp.Grid(olats, olons, oelevs, olafs)
    background = gridpp.full_gradient(igrid, ogrid, temp, egrad, lgrad, gridpp.Bilinear)
    d = R.device_downscaler(gridpp, igrid, ogrid, 1)
    composed = R.compose_full(d, temp, egrad, lgrad, ielevs, ilafs, oelevs, olafs).reshape(olats.shape)
    same_bits(background, composed)
    assert np.isfinite(background).all() and not np.array_equal(background, np.asarray(gridpp.bilinear(igrid, ogrid, temp)))
    S = 300
    plat, plon = 59.2 + 1.6 * rng.random(S), 9.2 + 2.6 * rng.random(S)
    points = gridpp.Points(plat, plon)
    pobs = rng.normal(5, 2, S).astype(F32)
    ratios = np.full(S, 0.3, F32)
    st = gridpp.BarnesStructure(30000)
    pbg = gridpp.nearest(ogrid, points, background)
    out = gridpp.optimal_interpolation(ogrid, background, points, pobs, ratios, pbg, st, 20)
    same_bits(out, gridpp.optimal_interpolation(ogrid, composed, points, pobs, ratios, gridpp.nearest(ogrid, points, composed), st, 20))
    assert np.isfinite(out).all() and np.abs(out - background).max() > 0.1


def test_full_size_1000x800_to_4000x4000():
    """Bilinear full_gradient, T = 3: bit-exact against the device composition, and against the oracle on 2000 sampled locations"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    Y, X, T, N = 1000, 800, 3, 4000
    lats, lons = np.meshgrid(np.linspace(55, 65, Y), np.linspace(5, 15, X), indexing="ij")
    ielevs = rng.uniform(0, 2000, (Y, X)).astype(F32)
    ilafs = rng.uniform(0, 1, (Y, X)).astype(F32)
    values = rng.normal(0, 5, (T, Y, X)).astype(F32)
    egrad = rng.normal(-0.0065, 0.002, (T, Y, X)).astype(F32)
    lgrad = rng.normal(2, 1, (T, Y, X)).astype(F32)
    igrid = gridpp.Grid(lats, lons, ielevs, ilafs)
    olats, olons = np.meshgrid(np.linspace(54.9, 65.1, N, dtype=F32), np.linspace(4.9, 15.1, N, dtype=F32), indexing="ij")
    oelevs = rng.uniform(0, 2000, (N, N)).astype(F32)
    olafs = rng.uniform(0, 1, (N, N)).astype(F32)
    ogrid = gridpp.Grid(olats, olons, oelevs, olafs)
    fused = gridpp.full_gradient(igrid, ogrid, values, egrad, lgrad, gridpp.Bilinear)
    assert fused.shape == (T, N, N)
    d = R.device_downscaler(gridpp, igrid, ogrid, 1)
    same_bits(fused, R.compose_full(d, values, egrad, lgrad, ielevs, ilafs, oelevs, olafs).reshape(T, N, N))
    iy, ix = rng.integers(0, N, 2000), rng.integers(0, N, 2000)
    do_, memo = R.oracle_downscaler(O, lats, lons, olats[iy, ix], olons[iy, ix], 1), {}
    do = lambda f: memo[id(f)] if id(f) in memo else memo.setdefault(id(f), do_(f))   # noqa: E731 (each field once)
    ref = R.compose_full(do, values, egrad, lgrad, ielevs, ilafs, oelevs[iy, ix], olafs[iy, ix])
    a = lambda f: np.abs(do(f)).astype(np.float64)   # noqa: E731
    bound = 4e-6 * (1 + a(values) + a(egrad) * (1 + oelevs[iy, ix] + a(ielevs)) + a(lgrad) * (1 + olafs[iy, ix] + a(ilafs)))
    assert close(fused[:, iy, ix], ref, bound) > 0.99
    assert np.mean(do(values) != R.oracle_downscaler(O, lats, lons, olats[iy, ix], olons[iy, ix], 0)(values)) > 0.9
