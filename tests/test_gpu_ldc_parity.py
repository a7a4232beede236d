"""local_distribution_correction on the device (gridpp_amd/csrc/ldc.hip) against the restatement of tests/ldc_ref.py.

The reference has one test of this function, a comparison between thread counts, and no numeric pin: parity is unpinned against
the reference, pinned only by the restatement of src/api/local_distribution_correction.cpp:33-203 with the tie rule "ties in
value are ordered by rho ascending" (tests/test_ldc_restatement.py pins the restatement by hand-derived answers).

Every branch condition depends on sorted values only, so every cell that does not take branch 4 (the two interpolations) must
equal the restatement bit for bit.  On branch-4 cells the one free quantity is the order of the float32 sum of rho:

    |got - ref| <= 1e-5 max(|ref|, 1e-3)

1e-5 relative is the project's parity tolerance.  Measured on the CPU when the function was specified: a
float64-accumulated cumulative sum against the sequential one moved the result by at most 5.4e-7 relative on tie-free data,
and by at most 2.1e-6 absolute on the data rounded to 0.5 mm -- the bound is about 20 times the effect.  No cell is left out.

Barnes and Cressman run on tie-free values and on the same values rounded to 0.5 mm (their device rho is bit-exact,
tests/test_gpu_staticcorr_parity.py).  Soar, a MultipleStructure with elevations and CrossValidation run on the tie-free set
only: the device exp is within one ulp of libm's there, and one ulp of rho may reorder a tie."""
import numpy as np
import pytest

from tests import ldc_ref as R

pytestmark = pytest.mark.gpu
F = np.float32


class Case:
    """a fixture, its handles on both sides and the restatement's candidates per structure (computed once, never changed)"""

    def __init__(self, rounded):
        import gridpp_amd as gridpp
        from oracle import oracle as O
        self.O, self.fx = O, R.FixtureA(rounded)
        self.g, self.p = self.fx.oracle_points(O)
        self.grid, self.points = self.fx.device_points(gridpp)
        self._cands = {}

    def cands(self, name, ora):
        if name not in self._cands:
            self._cands[name] = R.candidates(self.O, self.g, self.p, ora)
        return self._cands[name]


@pytest.fixture(scope="module")
def cases():
    return {False: Case(False), True: Case(True)}


def structures(gridpp, O):
    return {"Barnes": (gridpp.BarnesStructure(2500), O.Struct("Barnes", 2500)),
            "Cressman": (gridpp.CressmanStructure(6000), O.Struct("Cressman", 6000)),
            "Soar": (gridpp.SoarStructure(2500), O.Struct("Soar", 2500))}


def check(got, ref, tags):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == F and got.shape == ref.shape
    got, ref = got.ravel(), ref.ravel()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    four = tags == R.B4
    np.testing.assert_array_equal(got[~four].view(np.uint32), ref[~four].view(np.uint32))
    # a branch-4 cell may be NaN (a rho total of 0, tests/ldc_edge_cases.py): both sides are NaN there by the assertion above, and
    # NaN <= NaN would fail a cell that agrees; every other branch-4 cell is held to the bound
    four = four & ~np.isnan(ref)
    err = np.abs(got[four].astype(np.float64) - ref[four].astype(np.float64))
    bound = 1e-5 * np.maximum(np.abs(ref[four].astype(np.float64)), 1e-3)
    print("branch-4 cells: %d, max err / bound = %.3g" % (four.sum(), (err / bound).max() if four.any() else 0.0))
    assert np.all(err <= bound), (err / bound).max()


def test_the_fixture_reaches_every_branch(cases):
    import gridpp_amd as gridpp
    for rounded, c in cases.items():
        dev, ora = structures(gridpp, c.O)["Barnes"]
        fx = c.fx
        ref, tags, count = R.ldc(c.O, c.cands("Barnes", ora), fx.bg, fx.pobs, fx.pbg, fx.MINQ, fx.MAXQ, fx.MIN_POINTS)
        assert set(tags) == set(R.TAGS), set(R.TAGS) - set(tags)
        assert count.max() > 100 and (count < fx.MIN_POINTS).any()
        check(gridpp.local_distribution_correction(c.grid, fx.bg, c.points, fx.pobs, fx.pbg, dev, fx.MINQ, fx.MAXQ, fx.MIN_POINTS), ref, tags)


@pytest.mark.parametrize("min_points", [0, 5, 1000])
@pytest.mark.parametrize("quantiles", [(0.1, 0.9), (0.0, 1.0), (0.5, 0.5)])
@pytest.mark.parametrize("nT", [1, 3])
@pytest.mark.parametrize("kind", ["Barnes", "Cressman"])
@pytest.mark.parametrize("rounded", [False, True], ids=["tiefree", "rounded"])
def test_against_the_restatement(cases, rounded, kind, nT, quantiles, min_points):
    """nT = 1 goes through the 1-D overload"""
    import gridpp_amd as gridpp
    c = cases[rounded]
    fx = c.fx
    dev, ora = structures(gridpp, c.O)[kind]
    po, pb = (fx.pobs[0], fx.pbg[0]) if nT == 1 else (fx.pobs, fx.pbg)
    ref, tags, _ = R.ldc(c.O, c.cands(kind, ora), fx.bg, po, pb, quantiles[0], quantiles[1], min_points)
    check(gridpp.local_distribution_correction(c.grid, fx.bg, c.points, po, pb, dev, quantiles[0], quantiles[1], min_points), ref, tags)


def test_soar_multiple_and_cross_validation(cases):
    """tie-free values only (see the module's docstring); the MultipleStructure mixes kernels and has elevations to work on"""
    import gridpp_amd as gridpp
    O = cases[False].O
    fx = cases[False].fx
    rng = np.random.default_rng(3)
    gelev, pelev = rng.uniform(0, 400, fx.lats.shape), rng.uniform(0, 400, fx.px.size)
    g, p = O.Pts(fx.lats, fx.lons, gelev, ctype=1), O.Pts(fx.py, fx.px, pelev, ctype=1)
    grid = gridpp.Grid(fx.lats, fx.lons, gelev, ((),), gridpp.Cartesian)
    points = gridpp.Points(fx.py, fx.px, pelev, (), gridpp.Cartesian)
    soar_d, soar_o = structures(gridpp, O)["Soar"]
    barnes_d, barnes_o = structures(gridpp, O)["Barnes"]
    pairs = {"Soar": (soar_d, soar_o),
             "Multiple": (gridpp.MultipleStructure(gridpp.BarnesStructure(2500, 11, 22), gridpp.CressmanStructure(33, 300, 44),
                                                   gridpp.SoarStructure(55, 66, 0.5)),
                          O.Struct.multiple(O.Struct("Barnes", 2500, 11, 22), O.Struct("Cressman", 33, 300, 44), O.Struct("Soar", 55, 66, 0.5))),
             "CrossValidation": (gridpp.CrossValidation(barnes_d, 1500), barnes_o.cross_validation(1500))}
    for name, (dev, ora) in pairs.items():
        ref, tags, _ = R.ldc(O, R.candidates(O, g, p, ora), fx.bg, fx.pobs, fx.pbg, fx.MINQ, fx.MAXQ, fx.MIN_POINTS)
        assert (tags == R.B4).sum() > 50, name
        check(gridpp.local_distribution_correction(grid, fx.bg, points, fx.pobs, fx.pbg, dev, fx.MINQ, fx.MAXQ, fx.MIN_POINTS), ref, tags)


def test_the_order_of_the_stations_does_not_matter(cases):
    """rounded data: permuting the stations (and the columns of pobs / pbackground alike) changes the order the neighbours are met in;
    a plain sort by value would change the result with it (tests/test_ldc_restatement.py)"""
    import gridpp_amd as gridpp
    c = cases[True]
    fx = c.fx
    dev, ora = structures(gridpp, c.O)["Barnes"]
    ref, tags, _ = R.ldc(c.O, c.cands("Barnes", ora), fx.bg, fx.pobs, fx.pbg, fx.MINQ, fx.MAXQ, fx.MIN_POINTS)
    perm = np.random.default_rng(11).permutation(fx.px.size)
    points = gridpp.Points(fx.py[perm], fx.px[perm], (), (), gridpp.Cartesian)
    got = gridpp.local_distribution_correction(c.grid, fx.bg, points, fx.pobs[:, perm], fx.pbg[:, perm], dev, fx.MINQ, fx.MAXQ, fx.MIN_POINTS)
    check(got, ref, tags)


def test_the_hbm_path_and_the_chunked_fill(cases, monkeypatch):
    """fixture A with every cell on the path beyond the LDS bound, and with the keys filled in several chunks: the same bits"""
    import gridpp_amd as gridpp
    for rounded, c in cases.items():
        fx = c.fx
        dev, ora = structures(gridpp, c.O)["Barnes"]
        args = (c.grid, fx.bg, c.points, fx.pobs, fx.pbg, dev, fx.MINQ, fx.MAXQ, fx.MIN_POINTS)
        base = gridpp.local_distribution_correction(*args)
        ref, tags, count = R.ldc(c.O, c.cands("Barnes", ora), fx.bg, fx.pobs, fx.pbg, fx.MINQ, fx.MAXQ, fx.MIN_POINTS)
        monkeypatch.setenv("GPP_LDC_HBM", "1")
        hbm = gridpp.local_distribution_correction(*args)
        assert "GPP_LDC_HBM" in gridpp.active_overrides()
        check(hbm, ref, tags)
        np.testing.assert_array_equal(hbm.view(np.uint32), base.view(np.uint32))
        monkeypatch.delenv("GPP_LDC_HBM")
        assert count.sum() > 4 * 1000
        for cap in (1000, 300):
            monkeypatch.setenv("GPP_CSR_CAP", str(cap))
            np.testing.assert_array_equal(gridpp.local_distribution_correction(*args).view(np.uint32), base.view(np.uint32))
            monkeypatch.setenv("GPP_LDC_HBM", "1")
            np.testing.assert_array_equal(gridpp.local_distribution_correction(*args).view(np.uint32), base.view(np.uint32))
            monkeypatch.delenv("GPP_LDC_HBM")
        monkeypatch.delenv("GPP_CSR_CAP")


def test_a_large_count():
    """one row of 8 cells, 700 stations within 2 km, T = 4: 2 800 pairs per cell, beyond the LDS bound (512 pairs)"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    lons, lats = np.meshgrid(np.linspace(0, 1400, 8), [0.0])
    ang, rad = rng.uniform(0, 2 * np.pi, 700), 2000 * np.sqrt(rng.uniform(0, 1, 700))
    px, py = 700 + rad * np.cos(ang), rad * np.sin(ang)
    pobs, pbg = rng.gamma(0.6, 3, (4, 700)).astype(F), rng.gamma(0.6, 3, (4, 700)).astype(F)
    bg = np.array([[0.5, 1.0, 2.0, 4.0, 8.0, 0.05, 60.0, 3.0]], F)
    g, p = O.Pts(lats, lons, ctype=1), O.Pts(py, px, ctype=1)
    ref, tags, count = R.ldc(O, R.candidates(O, g, p, O.Struct("Barnes", 2500)), bg, pobs, pbg, 0.1, 0.9, 5)
    assert (count == 2800).all() and (tags == R.B4).sum() >= 5 and (tags == R.B3).any()
    grid = gridpp.Grid(lats, lons, ((),), ((),), gridpp.Cartesian)
    points = gridpp.Points(py, px, (), (), gridpp.Cartesian)
    check(gridpp.local_distribution_correction(grid, bg, points, pobs, pbg, gridpp.BarnesStructure(2500), 0.1, 0.9, 5), ref, tags)


def test_float64_lists_and_device_tensors(cases):
    import torch
    import gridpp_amd as gridpp
    c = cases[False]
    fx = c.fx
    dev, _ = structures(gridpp, c.O)["Barnes"]
    tail = (dev, fx.MINQ, fx.MAXQ, fx.MIN_POINTS)
    base = gridpp.local_distribution_correction(c.grid, fx.bg, c.points, fx.pobs, fx.pbg, *tail)
    got = gridpp.local_distribution_correction(c.grid, fx.bg.astype(np.float64), c.points, fx.pobs.astype(np.float64), fx.pbg.astype(np.float64), *tail)
    assert got.dtype == F and got.shape == tuple(c.grid.size())
    np.testing.assert_array_equal(got.view(np.uint32), base.view(np.uint32))
    got = gridpp.local_distribution_correction(c.grid, fx.bg.tolist(), c.points, fx.pobs.tolist(), fx.pbg.tolist(), *tail)
    np.testing.assert_array_equal(got.view(np.uint32), base.view(np.uint32))
    t = gridpp.local_distribution_correction(c.grid, torch.from_numpy(fx.bg).cuda(), c.points, torch.from_numpy(fx.pobs).cuda(),
                                             torch.from_numpy(fx.pbg).cuda(), *tail)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
    np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), base.view(np.uint32))


def test_geodetic():
    import gridpp_amd as gridpp
    from oracle import oracle as O
    rng = np.random.default_rng(9)
    lons, lats = np.meshgrid(10 + np.linspace(0, 0.2, 9), 60 + np.linspace(0, 0.2, 11))
    plat, plon = 60 + rng.uniform(0, 0.2, 50), 10 + rng.uniform(0, 0.2, 50)
    pobs, pbg = rng.gamma(0.6, 3, (2, 50)).astype(F), rng.gamma(0.6, 3, (2, 50)).astype(F)
    bg = rng.gamma(0.6, 3, lats.shape).astype(F)
    ref, tags, _ = R.ldc(O, R.candidates(O, O.Pts(lats, lons), O.Pts(plat, plon), O.Struct("Barnes", 2500)), bg, pobs, pbg, 0.1, 0.9, 5)
    assert (tags == R.B4).sum() > 20
    got = gridpp.local_distribution_correction(gridpp.Grid(lats, lons), bg, gridpp.Points(plat, plon), pobs, pbg, gridpp.BarnesStructure(2500), 0.1, 0.9, 5)
    check(got, ref, tags)


def test_empty_sets_and_refused_structures(cases):
    import gridpp_amd as gridpp
    c = cases[False]
    fx = c.fx
    dev, _ = structures(gridpp, c.O)["Barnes"]
    none = gridpp.Points((), (), (), (), gridpp.Cartesian)
    got = gridpp.local_distribution_correction(c.grid, fx.bg, none, np.zeros((3, 0), F), np.zeros((3, 0), F), dev, 0.1, 0.9, 5)
    np.testing.assert_array_equal(got.view(np.uint32), fx.bg.view(np.uint32))
    Y, X = c.grid.size()
    h = np.full((Y, X), 2500.0)
    h[0, 0] = 3000.0
    varying = gridpp.BarnesStructure(c.grid, h, np.zeros((Y, X)), np.zeros((Y, X)))
    with pytest.raises(RuntimeError, match="local_distribution_correction: spatially varying structure functions are not supported on the GPU path yet"):
        gridpp.local_distribution_correction(c.grid, fx.bg, c.points, fx.pobs, fx.pbg, varying, 0.1, 0.9, 5)
