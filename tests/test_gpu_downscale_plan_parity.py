"""The reusable downscaling plan (gridpp_amd.downscaling_plan, gridpp_amd/csrc/downscale_plan.hip) against the direct calls on the same
inputs, bit for bit: NaN matches NaN, every other float is identical (same_bits of tests/test_gpu_downscaling_parity.py).  The direct
calls are pinned to the oracle by tests/test_gpu_downscaling_parity.py, tests/test_gpu_bilinear_parity.py and
tests/test_gpu_bilinear_general.py.  Where a direct call raises "Problem with bilinear interpolation", the planned one must raise too."""
import functools
import gc

import numpy as np
import pytest

from tests import bilinear_cases as B
from tests.downscaling_ref import F32

pytestmark = pytest.mark.gpu
DISTORTED = "Problem with bilinear interpolation"


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert a.dtype == b.dtype == F32
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) or np.array_equal(a, b, equal_nan=True), \
        int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b)))))


def same_outcome(planned, direct):
    """both calls give the same bits, or both raise the error of a distorted box -> True when they raised"""
    try:
        want = direct()
    except RuntimeError as e:
        assert DISTORTED in str(e)
        with pytest.raises(RuntimeError, match=DISTORTED):
            planned()
        return True
    same_bits(planned(), want)
    return False


# ---- the case builder of tests/test_gpu_downscaling_parity.py (without its oracle side) ------------------------------------------------
def _mesh(kind, Y, X):
    if kind == "regular":
        return np.meshgrid(np.linspace(50.0, 52.0, Y), np.linspace(5.0, 8.0, X), indexing="ij")
    if kind == "warped":   # rotated, sheared, mildly curved
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
    def __init__(self, mesh, out_kind, T, seed, Y=41, X=53, ctype=None, n=3000):
        import gridpp_amd as gridpp
        rng = np.random.default_rng(seed)
        if isinstance(mesh, str):
            self.ctype = gridpp.Cartesian if mesh == "cartesian" else gridpp.Geodetic
            self.lats, self.lons = _mesh(mesh, Y, X)
        else:   # the mesh itself
            self.ctype = gridpp.Geodetic if ctype is None else ctype
            self.lats, self.lons = (np.asarray(a) for a in mesh)
            Y, X = self.lats.shape
        self.ielevs = _spoil(rng, rng.uniform(0, 1500, (Y, X)), 0.02, False)
        self.ilafs = _spoil(rng, rng.uniform(0, 1, (Y, X)), 0.02, False)
        lead = (T,) if T is not None else ()
        self.values = _spoil(rng, rng.normal(5, 3, lead + (Y, X)))
        self.egrad = _spoil(rng, rng.normal(-0.0065, 0.002, lead + (Y, X)))
        self.lgrad = _spoil(rng, rng.normal(2, 1, lead + (Y, X)))
        la, lo = self.lats, self.lons
        dla, dlo = la.max() - la.min(), lo.max() - lo.min()
        if out_kind == "grid":   # reaches 5 % outside the domain
            self.qlats, self.qlons = np.meshgrid(np.linspace(la.min() - 0.05 * dla, la.max() + 0.05 * dla, 37),
                                                 np.linspace(lo.min() - 0.05 * dlo, lo.max() + 0.05 * dlo, 43), indexing="ij")
        else:
            self.qlats = la.min() - 0.08 * dla + 1.16 * dla * rng.random(n)
            self.qlons = lo.min() - 0.08 * dlo + 1.16 * dlo * rng.random(n)
            k = min(150, n, la.size)
            self.qlats[:k], self.qlons[:k] = la.ravel()[:k], lo.ravel()[:k]   # grid nodes: s / t land on 0 or 1
        self.oelevs = _spoil(rng, rng.uniform(0, 1500, self.qlats.shape))
        self.olafs = _spoil(rng, rng.uniform(0, 1, self.qlats.shape))
        self.igrid = gridpp.Grid(self.lats, self.lons, self.ielevs, self.ilafs, type=self.ctype)
        if out_kind == "grid":
            self.out = gridpp.Grid(self.qlats, self.qlons, self.oelevs, self.olafs, type=self.ctype)
        else:
            self.out = gridpp.Points(self.qlats, self.qlons, self.oelevs, self.olafs, type=self.ctype)
        self.oshape = np.shape(self.qlats)

    def cube(self, E, seed):
        """(Y, X, E), every member spoiled on its own: one location mixes interpolated and nearest members"""
        rng = np.random.default_rng(seed)
        return _spoil(rng, rng.normal(5, 3, self.lats.shape + (E,)), 0.05)


@functools.lru_cache(maxsize=None)
def case(mesh, out_kind, T):
    return Case(mesh, out_kind, T, seed=300 + 7 * (T or 0) + len(mesh) + len(out_kind))


def check_methods(gridpp, c, ds, plan=None):
    """apply, simple_gradient and full_gradient (both gradients, the elevation only, neither) of one plan against the direct calls"""
    plan = plan or gridpp.downscaling_plan(c.igrid, c.out, ds)
    g, o, v = c.igrid, c.out, c.values
    same_outcome(lambda: plan.apply(v), lambda: gridpp.downscaling(g, o, v, ds))
    same_outcome(lambda: plan.simple_gradient(v, 0.0123), lambda: gridpp.simple_gradient(g, o, v, 0.0123, ds))
    for eg, lg in ((c.egrad, c.lgrad), (c.egrad, []), ([], [])):
        same_outcome(lambda: plan.full_gradient(v, eg, lg), lambda: gridpp.full_gradient(g, o, v, eg, lg, ds))
    return plan


# ---- geometry and method sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds", [0, 1], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("T", [None, 1, 3])
@pytest.mark.parametrize("out_kind", ["grid", "points"])
@pytest.mark.parametrize("mesh", ["regular", "warped", "cartesian"])
def test_geometry_and_method_sweep(mesh, out_kind, T, ds):
    import gridpp_amd as gridpp
    c = case(mesh, out_kind, T)
    plan = check_methods(gridpp, c, ds)
    assert plan.nbytes >= (16 if ds else 4) * int(np.prod(c.oshape))
    if ds:   # the case exercises the interpolation, not only the nearest-neighbour fallback, and locations outside the domain
        interpolated = np.asarray(plan.apply(c.values)) != np.asarray(gridpp.downscaling(c.igrid, c.out, c.values, gridpp.Nearest))
        assert 0.3 < np.mean(interpolated) < 1.0
        assert plan.distorted == 0


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 255, 256, 257])
def test_block_edges(nq):
    """output sizes around a wave and a workgroup of one location per lane; with 5 members a group of 4 lanes per location"""
    import gridpp_amd as gridpp
    c = Case("warped", "points", 2, seed=40 + nq, n=nq)
    cube = c.cube(5, nq)
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        plan = check_methods(gridpp, c, ds)
        assert plan.apply(c.values).shape == (2, nq)
        same_bits(plan.apply_cube(cube), np.moveaxis(gridpp.downscaling(c.igrid, c.out, np.moveaxis(cube, 2, 0), ds), 0, -1))


# ---- apply_cube ------------------------------------------------------------------------------------------------------------------------
MEMBERS = [1, 3, 4, 5, 16, 17, 32, 33, 50, 64, 65, 128, 129, 256, 257, 300]   # both sides of every 4 G, and past 256 where lanes loop
# an even number of members is read in pairs (Bilinear): G follows the number of pairs, so its boundaries sit at 8 G members
MEMBERS += [2, 34, 66, 130, 258, 512, 514, 600]


@functools.lru_cache(maxsize=None)
def cube_case(out_kind):
    return Case("warped", out_kind, None, seed=77, Y=19, X=23, n=700)


@pytest.mark.parametrize("E", MEMBERS)
def test_apply_cube_member_sweep(E):
    import gridpp_amd as gridpp
    c = cube_case("points")
    cube = c.cube(E, 1000 + E)
    levels = np.ascontiguousarray(np.moveaxis(cube, 2, 0))   # (E, Y, X) for the direct call
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        got = gridpp.downscaling_plan(c.igrid, c.out, ds).apply_cube(cube)
        assert got.shape == (700, E)
        same_bits(got, np.ascontiguousarray(np.moveaxis(gridpp.downscaling(c.igrid, c.out, levels, ds), 0, -1)))


@pytest.mark.parametrize("out_kind", ["grid", "points"])
def test_apply_cube_spoiled_members_plane_by_plane(out_kind):
    import gridpp_amd as gridpp
    c = cube_case(out_kind)
    E = 9
    cube = c.cube(E, 5)
    plan = gridpp.downscaling_plan(c.igrid, c.out, gridpp.Bilinear)
    got = plan.apply_cube(cube)
    assert got.shape == c.oshape + (E,)
    planes = [np.asarray(gridpp.downscaling(c.igrid, c.out, np.ascontiguousarray(cube[..., e]), gridpp.Bilinear)) for e in range(E)]
    for e in range(E):
        same_bits(np.ascontiguousarray(got[..., e]), planes[e])
    # one location mixes interpolated and nearest members
    near = np.stack([np.asarray(gridpp.downscaling(c.igrid, c.out, np.ascontiguousarray(cube[..., e]), gridpp.Nearest)) for e in range(E)], -1)
    is_nearest = (got.view(np.uint32) == near.view(np.uint32)).reshape(-1, E)
    assert np.any(is_nearest.any(axis=1) & ~is_nearest.all(axis=1))
    same_bits(gridpp.downscaling_plan(c.igrid, c.out, gridpp.Nearest).apply_cube(cube), near)


# ---- general quadrilaterals: the quadratic branch of the weights ----------------------------------------------------------------------------
GENERAL = [i for i in B.CASE_IDS if i.startswith("trapezoid")] + ["metres_6e5-flipY", "degrees-asis"]


@pytest.mark.parametrize("case_id", GENERAL)
def test_general_quadrilaterals(case_id):
    import gridpp_amd as gridpp
    g = B.case(case_id)
    assert B.classify(g.lats, g.lons)["parallelogram"] < (g.shape[0] - 1) * (g.shape[1] - 1)   # some boxes take the general solve
    rng = np.random.default_rng(B.CASE_IDS.index(case_id))
    igrid = gridpp.Grid(g.lats, g.lons, rng.uniform(0, 1500, g.shape), rng.uniform(0, 1, g.shape), type=g.ctype)
    out = gridpp.Points(g.qlat, g.qlon, rng.uniform(0, 1500, g.qlat.size), rng.uniform(0, 1, g.qlat.size), type=g.ctype)
    plan = gridpp.downscaling_plan(igrid, out, gridpp.Bilinear)
    stack = np.stack([g.values, g.linear])
    same_outcome(lambda: plan.apply(g.values), lambda: gridpp.downscaling(igrid, out, g.values, gridpp.Bilinear))
    same_outcome(lambda: plan.apply(stack), lambda: gridpp.downscaling(igrid, out, stack, gridpp.Bilinear))
    same_outcome(lambda: np.moveaxis(plan.apply_cube(np.ascontiguousarray(np.moveaxis(stack, 0, -1))), -1, 0),
                 lambda: gridpp.downscaling(igrid, out, stack, gridpp.Bilinear))
    same_outcome(lambda: plan.full_gradient(stack, stack[::-1], stack), lambda: gridpp.full_gradient(igrid, out, stack, stack[::-1], stack, gridpp.Bilinear))
    same_outcome(lambda: plan.simple_gradient(g.values, -0.0065), lambda: gridpp.simple_gradient(igrid, out, g.values, -0.0065, gridpp.Bilinear))


# ---- degenerate inputs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 17), (17, 1)])
def test_grids_of_one_row_or_column_have_no_box(shape):
    import gridpp_amd as gridpp
    Y, X = shape
    lats, lons = np.meshgrid(np.linspace(60, 61, Y) if Y > 1 else [60.0], np.linspace(10, 12, X) if X > 1 else [10.0], indexing="ij")
    c = Case((lats, lons), "points", 2, seed=3, n=300)
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        check_methods(gridpp, c, ds)
    cube = c.cube(6, 1)
    bil, near = (gridpp.downscaling_plan(c.igrid, c.out, ds) for ds in (gridpp.Bilinear, gridpp.Nearest))
    same_bits(bil.apply(c.values), near.apply(c.values))   # all nearest
    same_bits(bil.apply_cube(cube), near.apply_cube(cube))
    same_bits(bil.apply_cube(cube), np.moveaxis(gridpp.downscaling(c.igrid, c.out, np.moveaxis(cube, 2, 0), gridpp.Bilinear), 0, -1))


def test_empty_input_output_and_levels():
    import gridpp_amd as gridpp
    c = case("warped", "points", 3)
    nq = c.qlats.size
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        # an empty input grid: all NaN, as the direct calls
        plan = gridpp.downscaling_plan(gridpp.Grid(), c.out, ds)
        for got, shape in ((plan.apply(np.zeros((3, 0, 0))), (3, nq)), (plan.apply_cube(np.zeros((0, 0, 4))), (nq, 4)),
                           (plan.full_gradient(np.zeros((3, 0, 0)), [], []), (3, nq)), (plan.simple_gradient(np.zeros((3, 0, 0)), 0.5), (3, nq))):
            assert got.shape == shape and got.dtype == F32 and np.all(np.isnan(got))
        same_bits(plan.apply(np.zeros((3, 0, 0))), gridpp.downscaling(gridpp.Grid(), c.out, np.zeros((3, 0, 0)), ds))
        # an empty output
        for empty, oshape in ((gridpp.Points([], [], type=c.ctype), (0,)), (gridpp.Grid(type=c.ctype), (0, 0))):
            plan = gridpp.downscaling_plan(c.igrid, empty, ds)
            assert plan.apply(c.values).shape == (3,) + oshape == np.shape(gridpp.downscaling(c.igrid, empty, c.values, ds))
            assert plan.apply(c.values[0]).shape == oshape
            assert plan.apply_cube(np.zeros(c.lats.shape + (4,), F32)).shape == oshape + (4,)
            assert plan.simple_gradient(c.values, 0.5).shape == (3,) + oshape
            assert plan.full_gradient(c.values, c.egrad, c.lgrad).shape == (3,) + oshape
        # no levels, no members
        plan = gridpp.downscaling_plan(c.igrid, c.out, ds)
        none = np.zeros((0,) + c.lats.shape, F32)
        assert plan.apply(none).shape == (0, nq) == np.shape(gridpp.downscaling(c.igrid, c.out, none, ds))
        assert plan.full_gradient(none, none, none).shape == (0, nq) and plan.simple_gradient(none, 1.0).shape == (0, nq)
        assert plan.apply_cube(np.zeros(c.lats.shape + (0,), F32)).shape == (nq, 0)


# ---- the error of a distorted box keeps its condition -------------------------------------------------------------------------------------
def test_distorted_box_raises_where_the_direct_call_raises():
    """the millidegree kite of test_distorted_box_raises_where_bilinear_raises: it passes both 'parallel' tests of the weights; the
    location near the far corner is rejected by bilinear, the one near the well-behaved corner is not"""
    import gridpp_amd as gridpp
    lats = np.array([[0, -0.002], [0.001, 0.001]])
    lons = np.array([[0, 0.003], [0, 0.001]])
    grid = gridpp.Grid(lats, lons, np.array([[1, 2], [3, 4]]), np.array([[0.1, 0.2], [0.3, 0.4]]), type=gridpp.Cartesian)
    bad = gridpp.Points([-0.0015], [0.0025], [10], [0.5], type=gridpp.Cartesian)
    good = gridpp.Points([0.0005], [0.0005], [10], [0.5], type=gridpp.Cartesian)
    vals = np.array([[0, 1], [2, 3]], F32)
    nan = np.full((2, 2), np.nan, F32)
    B_, N_ = gridpp.Bilinear, gridpp.Nearest

    def methods(plan, g, p, v, ds):
        return [(lambda: plan.apply(v), lambda: gridpp.downscaling(g, p, v, ds)),
                (lambda: plan.apply(np.stack([v, v])), lambda: gridpp.downscaling(g, p, np.stack([v, v]), ds)),
                (lambda: plan.apply_cube(np.ascontiguousarray(v[..., None]))[..., 0], lambda: gridpp.downscaling(g, p, v, ds)),
                (lambda: plan.simple_gradient(v, 1.0), lambda: gridpp.simple_gradient(g, p, v, 1.0, ds)),
                (lambda: plan.full_gradient(v, vals, vals), lambda: gridpp.full_gradient(g, p, v, vals, vals, ds)),
                (lambda: plan.full_gradient(v, vals, []), lambda: gridpp.full_gradient(g, p, v, vals, [], ds)),
                (lambda: plan.full_gradient(v, [], []), lambda: gridpp.full_gradient(g, p, v, [], [], ds))]

    plan_bad = gridpp.downscaling_plan(grid, bad, B_)    # construction succeeds
    plan_good = gridpp.downscaling_plan(grid, good, B_)
    assert plan_bad.distorted == 1 and plan_good.distorted == 0
    # every method raises for the bad point, as its direct call does; none raises for the good point
    assert all(same_outcome(*m) for m in methods(plan_bad, grid, bad, vals, B_))
    assert not any(same_outcome(*m) for m in methods(plan_good, grid, good, vals, B_))
    # all-NaN values: apply has no field with four valid corners and does not raise; the gradients still downscale the elevations
    raised = [same_outcome(*m) for m in methods(plan_bad, grid, bad, nan, B_)]
    assert raised == [False, False, False, True, True, True, False]
    assert np.all(np.isnan(plan_bad.apply(nan)))
    # a gradient whose term is switched off (no valid elevation to difference) is still downscaled by the reference, and raises
    noelev = gridpp.Grid(lats, lons, type=gridpp.Cartesian)
    plan_noelev = gridpp.downscaling_plan(noelev, bad, B_)
    raised = [same_outcome(*m) for m in methods(plan_noelev, noelev, bad, nan, B_)]
    assert raised == [False, False, False, False, True, True, False]
    # a Nearest plan never raises
    plan_near = gridpp.downscaling_plan(grid, bad, N_)
    assert plan_near.distorted == 0
    assert not any(same_outcome(*m) for m in methods(plan_near, grid, bad, vals, N_))
    # the plan is usable after an apply that raised
    with pytest.raises(RuntimeError, match=r"s=.* and t=.* are outside"):
        plan_bad.apply(vals)
    assert not same_outcome(lambda: plan_bad.apply(nan), lambda: gridpp.downscaling(grid, bad, nan, B_))


# ---- memory and lifetime ---------------------------------------------------------------------------------------------------------------
def test_plan_outlives_its_grids_and_release():
    import gridpp_amd as gridpp
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        c = Case("warped", "grid", 2, seed=21)
        cube = c.cube(5, 2)
        want = [gridpp.downscaling(c.igrid, c.out, c.values, ds), gridpp.full_gradient(c.igrid, c.out, c.values, c.egrad, c.lgrad, ds),
                gridpp.simple_gradient(c.igrid, c.out, c.values, 0.3, ds), gridpp.downscaling(c.igrid, c.out, np.moveaxis(cube, 2, 0), ds)]
        plan = gridpp.downscaling_plan(c.igrid, c.out, ds)
        values, egrad, lgrad = c.values, c.egrad, c.lgrad
        c.igrid = c.out = None
        del c
        gc.collect()
        same_bits(plan.apply(values), want[0])
        same_bits(plan.full_gradient(values, egrad, lgrad), want[1])
        same_bits(plan.simple_gradient(values, 0.3), want[2])
        same_bits(np.moveaxis(plan.apply_cube(cube), -1, 0), want[3])
        assert plan.nbytes > 0
        plan.release()
        plan.release()   # twice is fine
        for use in (lambda: plan.apply(values), lambda: plan.apply_cube(cube), lambda: plan.simple_gradient(values, 0.3),
                    lambda: plan.full_gradient(values, egrad, lgrad), lambda: plan.nbytes, lambda: plan.distorted):
            with pytest.raises(RuntimeError, match="the plan was released"):
                use()


def test_device_tensors_and_float64_inputs():
    import torch
    import gridpp_amd as gridpp
    c = Case("warped", "grid", 4, seed=9)
    cube = c.cube(17, 3)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        plan = gridpp.downscaling_plan(c.igrid, c.out, ds)
        pairs = [(plan.apply(dev(c.values)), plan.apply(c.values)), (plan.apply_cube(dev(cube)), plan.apply_cube(cube)),
                 (plan.simple_gradient(dev(c.values), 0.5), plan.simple_gradient(c.values, 0.5)),
                 (plan.full_gradient(dev(c.values), dev(c.egrad), dev(c.lgrad)), plan.full_gradient(c.values, c.egrad, c.lgrad))]
        for got, host in pairs:
            assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == host.shape
            same_bits(got.cpu().numpy(), host)
        same_bits(pairs[0][1], gridpp.downscaling(c.igrid, c.out, c.values, ds))
        # an even number of members in a tensor that starts 4 bytes off an 8-byte boundary: no paired loads
        even = np.ascontiguousarray(cube[..., :16])
        flat = torch.empty(even.size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = dev(even).reshape(-1)
        offset = flat[1:].view(even.shape)
        assert offset.data_ptr() % 8 == 4 and offset.is_contiguous()
        same_bits(plan.apply_cube(offset).cpu().numpy(), plan.apply_cube(even))
        # mixing host and device field arguments
        with pytest.raises(ValueError):
            plan.full_gradient(dev(c.values), c.egrad, c.lgrad)
        with pytest.raises(ValueError):
            plan.full_gradient(c.values, dev(c.egrad), c.lgrad)
        # small float64 arrays are converted by numpy
        same_bits(plan.apply(c.values.astype(np.float64)), pairs[0][1])
        same_bits(plan.apply_cube(cube.astype(np.float64)), pairs[1][1])
    # float64 numpy inputs of >= 1 Mi elements are cast on the device: the same result as float32-cast inputs
    rng = np.random.default_rng(3)
    Y, X, T = 256, 512, 8
    lats, lons = _mesh("regular", Y, X)
    g = gridpp.Grid(lats, lons, rng.uniform(0, 800, (Y, X)), rng.uniform(0, 1, (Y, X)))
    o = gridpp.Points(50 + 2 * rng.random(5000), 5 + 3 * rng.random(5000), rng.uniform(0, 800, 5000), rng.uniform(0, 1, 5000))
    v, e, l_ = rng.normal(0, 3, (T, Y, X)), rng.normal(-0.006, 0.001, (T, Y, X)), rng.normal(1, 1, (T, Y, X))
    wide = np.ascontiguousarray(np.moveaxis(v, 0, -1))
    assert v.size >= 1 << 20 and v.dtype == wide.dtype == np.float64
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        plan = gridpp.downscaling_plan(g, o, ds)
        same_bits(plan.apply(v), gridpp.downscaling(g, o, v.astype(F32), ds))
        same_bits(plan.apply_cube(wide), np.moveaxis(gridpp.downscaling(g, o, v.astype(F32), ds), 0, -1))
        same_bits(plan.full_gradient(v, e, l_), gridpp.full_gradient(g, o, v.astype(F32), e.astype(F32), l_.astype(F32), ds))
        same_bits(plan.simple_gradient(v, 0.25), gridpp.simple_gradient(g, o, v.astype(F32), 0.25, ds))
