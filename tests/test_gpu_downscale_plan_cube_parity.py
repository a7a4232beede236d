"""The cube-layout gradients of the reusable downscaling plan (DownscalingPlan.simple_gradient_cube / full_gradient_cube,
k_plan_gradient_cube of gridpp_amd/csrc/downscale_plan.hip, the gradient terms of downscale_loc.h on a planned locator) against the
direct simple_gradient / full_gradient (k_downscale: the same terms on a direct locator) on the np.moveaxis-ed
(E, Y, X) arrays, a gradient shared by the members repeated per level: bit for bit, and raising "Problem with bilinear interpolation"
exactly where the direct call raises.  The direct calls are pinned to the oracle by tests/test_gpu_downscaling_parity.py."""
import functools
import gc

import numpy as np
import pytest

from tests import bilinear_cases as B
from tests.downscaling_ref import F32
from tests.test_gpu_downscale_plan_parity import GENERAL, Case, cube_case, same_bits, same_outcome

pytestmark = pytest.mark.gpu

# both sides of every group boundary of the scalar loads (4 G members) and of the paired loads (8 G), and past 256 / 512 where lanes loop
MEMBERS = [1, 2, 3, 5, 16, 17, 32, 33, 34, 50, 64, 65, 66, 129, 130, 257, 258, 600]
PER_MEMBER = [1, 2, 16, 17, 32, 33, 34, 64, 65, 66, 129, 130, 257, 258, 600]


def levels(a):
    """(..., E) -> (E, ...) for the direct call"""
    return np.ascontiguousarray(np.moveaxis(np.asarray(a), -1, 0))


def members_last(a):
    return np.ascontiguousarray(np.moveaxis(np.asarray(a), 0, -1))


def per_level(g, E):
    """a gradient of a cube call as the direct call on (E, Y, X) takes it: a shared field repeated per level"""
    if g is None or np.size(g) == 0:
        return []
    g = np.asarray(g)
    return levels(g) if g.ndim == 3 else np.ascontiguousarray(np.broadcast_to(g, (E,) + g.shape))


def direct_full(gridpp, igrid, out, cube, eg, lg, ds):
    E = cube.shape[-1]
    return members_last(gridpp.full_gradient(igrid, out, levels(cube), per_level(eg, E), per_level(lg, E), ds))


def direct_simple(gridpp, igrid, out, cube, gradient, ds):
    return members_last(gridpp.simple_gradient(igrid, out, levels(cube), gradient, ds))


def check_full(gridpp, plan, c, cube, eg, lg, ds):
    got = plan.full_gradient_cube(cube, eg, lg)
    same_bits(got, direct_full(gridpp, c.igrid, c.out, cube, eg, lg, ds))
    return got


@functools.lru_cache(maxsize=None)
def plans(out_kind):
    import gridpp_amd as gridpp
    c = cube_case(out_kind)
    return c, {ds: gridpp.downscaling_plan(c.igrid, c.out, ds) for ds in (gridpp.Nearest, gridpp.Bilinear)}


# ---- member counts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", MEMBERS)
def test_member_sweep(E):
    import gridpp_amd as gridpp
    c, by_ds = plans("points")
    cube = c.cube(E, 2000 + E)
    for ds, plan in by_ds.items():
        got = check_full(gridpp, plan, c, cube, c.egrad, c.lgrad, ds)
        assert got.shape == (700, E)
        same_bits(plan.simple_gradient_cube(cube, -0.0065), direct_simple(gridpp, c.igrid, c.out, cube, -0.0065, ds))
        if E in PER_MEMBER:
            check_full(gridpp, plan, c, cube, c.cube(E, 3000 + E), c.cube(E, 4000 + E), ds)


# ---- gradient forms, on the grid output and on the points, with an odd and an even member count -------------------------------------------
@pytest.mark.parametrize("E", [9, 10])
@pytest.mark.parametrize("out_kind", ["grid", "points"])
def test_gradient_forms(out_kind, E):
    import gridpp_amd as gridpp
    c, by_ds = plans(out_kind)
    cube, ecube, lcube = c.cube(E, 11), c.cube(E, 12), c.cube(E, 13)
    forms = [(c.egrad, c.lgrad), (c.egrad, []), ([], c.lgrad), ([], []), (None, None), (c.egrad, lcube), (ecube, c.lgrad), (ecube, lcube),
             (ecube, []), ([], lcube)]
    for ds, plan in by_ds.items():
        for eg, lg in forms:
            got = check_full(gridpp, plan, c, cube, eg, lg, ds)
            assert got.shape == c.oshape + (E,)
        same_bits(plan.simple_gradient_cube(cube, 0.0123), direct_simple(gridpp, c.igrid, c.out, cube, 0.0123, ds))
        same_bits(plan.full_gradient_cube(cube, [], []), plan.apply_cube(cube) + F32(0))   # no term: v + (0 + 0)
    # locations outside the domain take the nearest neighbour for every member and field
    outside = ((c.qlats < c.lats.min()) | (c.qlats > c.lats.max()) | (c.qlons < c.lons.min()) | (c.qlons > c.lons.max())).ravel()
    assert outside.sum() > 10
    bil, near = (np.asarray(by_ds[ds].full_gradient_cube(cube, ecube, c.lgrad)).reshape(-1, E) for ds in (gridpp.Bilinear, gridpp.Nearest))
    same_bits(bil[outside], near[outside])
    assert not np.array_equal(bil[~outside], near[~outside], equal_nan=True)


# ---- location counts around a wave and a workgroup of G lanes per location --------------------------------------------------------------------
@pytest.mark.parametrize("nq,E", [(1, 5), (63, 5), (64, 5), (65, 5), (257, 5), (31, 50), (32, 50), (33, 50)])
def test_location_counts(nq, E):
    import gridpp_amd as gridpp
    c = Case("warped", "points", None, seed=40 + nq, Y=19, X=23, n=nq)
    cube = c.cube(E, nq)
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        plan = gridpp.downscaling_plan(c.igrid, c.out, ds)
        assert check_full(gridpp, plan, c, cube, c.egrad, c.lgrad, ds).shape == (nq, E)
        check_full(gridpp, plan, c, cube, c.cube(E, nq + 1), c.lgrad, ds)
        same_bits(plan.simple_gradient_cube(cube, 0.5), direct_simple(gridpp, c.igrid, c.out, cube, 0.5, ds))


# ---- spoiled inputs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_kind", ["grid", "points"])
def test_spoiled_inputs_mix_members_and_switch_terms_off(out_kind):
    import gridpp_amd as gridpp
    c, by_ds = plans(out_kind)
    E = 9
    cube, ecube = c.cube(E, 5), c.cube(E, 6)
    plan, near = by_ds[gridpp.Bilinear], by_ds[gridpp.Nearest]
    both = check_full(gridpp, plan, c, cube, ecube, c.lgrad, gridpp.Bilinear).reshape(-1, E)
    # plane by plane against the direct 2-D call as well
    for e in (0, E - 1):
        same_bits(both[:, e].reshape(c.oshape), gridpp.full_gradient(c.igrid, c.out, np.ascontiguousarray(cube[..., e]),
                                                                     np.ascontiguousarray(ecube[..., e]), c.lgrad, gridpp.Bilinear))
    # some location mixes interpolated and nearest members of the values
    is_nearest = (np.asarray(plan.apply_cube(cube)).view(np.uint32) == np.asarray(near.apply_cube(cube)).view(np.uint32)).reshape(-1, E)
    assert np.any(is_nearest.any(axis=1) & ~is_nearest.all(axis=1))
    # some location has its elevation (laf) term switched off by an invalid oelev / d(ielev) (olaf / d(ilaf)): there, and only because
    # of that, the result is the one of a call without that gradient
    valid = lambda a: np.isfinite(np.asarray(a)).ravel()   # noqa: E731
    e_off = ~(valid(c.oelevs) & valid(plan.apply(c.ielevs)))
    l_off = ~(valid(c.olafs) & valid(plan.apply(c.ilafs)))
    assert (~valid(c.oelevs)).any() and (valid(c.oelevs) & ~valid(plan.apply(c.ielevs))).any()
    assert (~valid(c.olafs)).any() and (valid(c.olafs) & ~valid(plan.apply(c.ilafs))).any()
    no_elev = np.asarray(plan.full_gradient_cube(cube, [], c.lgrad)).reshape(-1, E)
    no_laf = np.asarray(plan.full_gradient_cube(cube, ecube, [])).reshape(-1, E)
    same_bits(both[e_off], no_elev[e_off])
    same_bits(both[l_off], no_laf[l_off])
    assert not np.array_equal(both[~e_off], no_elev[~e_off], equal_nan=True)
    assert not np.array_equal(both[~l_off], no_laf[~l_off], equal_nan=True)


# ---- other meshes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["regular", "cartesian"])
def test_other_mesh_kinds(mesh):
    import gridpp_amd as gridpp
    c = Case(mesh, "grid", None, seed=5, Y=19, X=23)
    cube = c.cube(6, 1)
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        plan = gridpp.downscaling_plan(c.igrid, c.out, ds)
        check_full(gridpp, plan, c, cube, c.egrad, c.cube(6, 2), ds)
        same_bits(plan.simple_gradient_cube(cube, 0.3), direct_simple(gridpp, c.igrid, c.out, cube, 0.3, ds))


def test_a_general_quadrilateral_mesh():
    import gridpp_amd as gridpp
    g = B.case(GENERAL[0])
    rng = np.random.default_rng(1)
    igrid = gridpp.Grid(g.lats, g.lons, rng.uniform(0, 1500, g.shape), rng.uniform(0, 1, g.shape), type=g.ctype)
    out = gridpp.Points(g.qlat, g.qlon, rng.uniform(0, 1500, g.qlat.size), rng.uniform(0, 1, g.qlat.size), type=g.ctype)
    plan = gridpp.downscaling_plan(igrid, out, gridpp.Bilinear)
    cube = np.ascontiguousarray(np.stack([g.values, g.linear, g.values[::-1, ::-1], g.linear], -1).astype(F32))
    grad = np.ascontiguousarray(cube[..., ::-1])
    same_outcome(lambda: plan.full_gradient_cube(cube, grad, g.linear), lambda: direct_full(gridpp, igrid, out, cube, grad, g.linear, gridpp.Bilinear))
    same_outcome(lambda: plan.simple_gradient_cube(cube, -0.0065), lambda: direct_simple(gridpp, igrid, out, cube, -0.0065, gridpp.Bilinear))


# ---- degenerate inputs ---------------------------------------------------------------------------------------------------------------------
def test_empty_grid_members_and_outputs():
    import gridpp_amd as gridpp
    c, _ = plans("points")
    nq = c.qlats.size
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        # an empty input grid: all NaN
        plan = gridpp.downscaling_plan(gridpp.Grid(), c.out, ds)
        none = np.zeros((0, 0, 4))
        for got in (plan.simple_gradient_cube(none, 0.5), plan.full_gradient_cube(none, [], []), plan.full_gradient_cube(none, none, np.zeros((0, 0)))):
            assert got.shape == (nq, 4) and got.dtype == F32 and np.all(np.isnan(got))
        # an empty output
        for empty, oshape in ((gridpp.Points([], [], type=c.ctype), (0,)), (gridpp.Grid(type=c.ctype), (0, 0))):
            plan = gridpp.downscaling_plan(c.igrid, empty, ds)
            cube = np.zeros(c.lats.shape + (4,), F32)
            assert plan.simple_gradient_cube(cube, 0.5).shape == oshape + (4,)
            assert plan.full_gradient_cube(cube, c.egrad, cube).shape == oshape + (4,)
        # no members
        plan = gridpp.downscaling_plan(c.igrid, c.out, ds)
        none = np.zeros(c.lats.shape + (0,), F32)
        assert plan.simple_gradient_cube(none, 1.0).shape == (nq, 0)
        assert plan.full_gradient_cube(none, c.egrad, none).shape == (nq, 0)


# ---- the error of a distorted box keeps its condition --------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [3, 4])
def test_distorted_box_raises_where_the_direct_call_raises(E):
    """the millidegree kite of tests/test_gpu_downscale_plan_parity.py (one location with bad weights): the planned cube call raises if and
    only if the direct call on the permuted arrays does -- when some downscaled field has four valid corners there"""
    import gridpp_amd as gridpp
    lats = np.array([[0, -0.002], [0.001, 0.001]])
    lons = np.array([[0, 0.003], [0, 0.001]])
    grid = gridpp.Grid(lats, lons, np.array([[1, 2], [3, 4]]), np.array([[0.1, 0.2], [0.3, 0.4]]), type=gridpp.Cartesian)
    noelev = gridpp.Grid(lats, lons, type=gridpp.Cartesian)
    bad = gridpp.Points([-0.0015], [0.0025], [10], [0.5], type=gridpp.Cartesian)
    good = gridpp.Points([0.0005], [0.0005], [10], [0.5], type=gridpp.Cartesian)
    ds = gridpp.Bilinear
    field = np.array([[0, 1], [2, 3]], F32)
    nan2, nan3 = np.full((2, 2), np.nan, F32), np.full((2, 2, E), np.nan, F32)
    ok3 = np.ascontiguousarray(np.repeat(field[..., None], E, -1))
    one = nan3.copy()
    one[..., E - 1] = field   # only the last member has four valid corners

    def full(g, p, plan, v, eg, lg):
        return same_outcome(lambda: plan.full_gradient_cube(v, eg, lg), lambda: direct_full(gridpp, g, p, v, eg, lg, ds))

    def simple(g, p, plan, v):
        return same_outcome(lambda: plan.simple_gradient_cube(v, 1.0), lambda: direct_simple(gridpp, g, p, v, 1.0, ds))

    plan_bad, plan_good, plan_noelev = (gridpp.downscaling_plan(g, p, ds) for g, p in ((grid, bad), (grid, good), (noelev, bad)))
    assert plan_bad.distorted == 1 and plan_good.distorted == 0 and plan_noelev.distorted == 1
    # valid everything: raises for the bad point, not for the good one
    assert full(grid, bad, plan_bad, ok3, field, ok3) and simple(grid, bad, plan_bad, ok3)
    assert not full(grid, good, plan_good, ok3, field, ok3) and not simple(grid, good, plan_good, ok3)
    # only a gradient has four valid corners there (no elevations or lafs on the grid: its term is switched off, it raises all the same)
    assert full(noelev, bad, plan_noelev, nan3, field, []) and full(noelev, bad, plan_noelev, nan3, [], field)
    assert full(noelev, bad, plan_noelev, nan3, one, nan2) and full(noelev, bad, plan_noelev, nan3, nan2, one)
    assert not full(noelev, bad, plan_noelev, nan3, nan3, nan2) and not full(noelev, bad, plan_noelev, nan3, nan2, nan3)
    # only the input elevations (lafs) have four valid corners there: downscaled whenever their gradient is present
    assert full(grid, bad, plan_bad, nan3, nan2, []) and full(grid, bad, plan_bad, nan3, [], nan3) and simple(grid, bad, plan_bad, nan3)
    assert not full(grid, bad, plan_bad, nan3, [], [])
    assert not simple(noelev, bad, plan_noelev, nan3)
    # only one member of the values does
    assert full(noelev, bad, plan_noelev, one, [], []) and simple(noelev, bad, plan_noelev, one)
    assert full(noelev, bad, plan_noelev, one, nan2, nan3)
    assert not full(noelev, bad, plan_noelev, nan3, [], [])
    # a Nearest plan never raises, and the plan is usable after a call that raised
    near = gridpp.downscaling_plan(grid, bad, gridpp.Nearest)
    same_bits(near.full_gradient_cube(ok3, field, ok3), members_last(gridpp.full_gradient(grid, bad, levels(ok3), per_level(field, E), levels(ok3), gridpp.Nearest)))
    with pytest.raises(RuntimeError, match=r"s=.* and t=.* are outside"):
        plan_bad.full_gradient_cube(ok3, field, ok3)
    assert not full(grid, bad, plan_bad, nan3, [], [])


# ---- alignment, types, memory, lifetime ------------------------------------------------------------------------------------------------------
def test_device_tensors_alignment_and_float64_inputs():
    import torch
    import gridpp_amd as gridpp
    c, by_ds = plans("grid")
    E = 16
    cube, ecube = c.cube(E, 3), c.cube(E, 4)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731

    def off_by_one_float(a):
        flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = dev(a).reshape(-1)
        t = flat[1:].view(a.shape)
        assert t.data_ptr() % 8 == 4 and t.is_contiguous()
        return t

    for ds, plan in by_ds.items():
        host = plan.full_gradient_cube(cube, ecube, c.lgrad)
        same_bits(host, direct_full(gridpp, c.igrid, c.out, cube, ecube, c.lgrad, ds))
        got = plan.full_gradient_cube(dev(cube), dev(ecube), dev(c.lgrad))
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == host.shape
        same_bits(got.cpu().numpy(), host)
        simple = plan.simple_gradient_cube(dev(cube), 0.5)
        assert simple.is_cuda
        same_bits(simple.cpu().numpy(), plan.simple_gradient_cube(cube, 0.5))
        # an even number of members in a tensor that starts 4 bytes off an 8-byte boundary: the scalar path, the same bits --
        # the values, a per-member gradient, and both
        same_bits(plan.full_gradient_cube(off_by_one_float(cube), dev(ecube), dev(c.lgrad)).cpu().numpy(), host)
        same_bits(plan.full_gradient_cube(dev(cube), off_by_one_float(ecube), dev(c.lgrad)).cpu().numpy(), host)
        same_bits(plan.full_gradient_cube(off_by_one_float(cube), off_by_one_float(ecube), dev(c.lgrad)).cpu().numpy(), host)
        same_bits(plan.simple_gradient_cube(off_by_one_float(cube), 0.5).cpu().numpy(), simple.cpu().numpy())
        # host and device arguments do not mix
        with pytest.raises(ValueError):
            plan.full_gradient_cube(dev(cube), ecube, c.lgrad)
        with pytest.raises(ValueError):
            plan.full_gradient_cube(cube, ecube, dev(c.lgrad))
        # float64 inputs are converted
        same_bits(plan.full_gradient_cube(cube.astype(np.float64), ecube.astype(np.float64), c.lgrad.astype(np.float64)), host)
        same_bits(plan.simple_gradient_cube(cube.astype(np.float64), 0.5), plan.simple_gradient_cube(cube, 0.5))


def test_large_float64_inputs_are_cast_on_the_device():
    """float64 numpy inputs of >= 1 Mi elements take the device-side cast: the same result as float32-cast inputs"""
    import gridpp_amd as gridpp
    rng = np.random.default_rng(3)
    Y, X, E = 128, 256, 32
    lats, lons = np.meshgrid(np.linspace(50.0, 52.0, Y), np.linspace(5.0, 8.0, X), indexing="ij")
    g = gridpp.Grid(lats, lons, rng.uniform(0, 800, (Y, X)), rng.uniform(0, 1, (Y, X)))
    o = gridpp.Points(50 + 2 * rng.random(2000), 5 + 3 * rng.random(2000), rng.uniform(0, 800, 2000), rng.uniform(0, 1, 2000))
    v, e, l_ = rng.normal(0, 3, (Y, X, E)), rng.normal(-0.006, 0.001, (Y, X, E)), rng.normal(1, 1, (Y, X))
    assert v.size >= 1 << 20 and v.dtype == np.float64
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        plan = gridpp.downscaling_plan(g, o, ds)
        same_bits(plan.full_gradient_cube(v, e, l_), plan.full_gradient_cube(v.astype(F32), e.astype(F32), l_.astype(F32)))
        same_bits(plan.full_gradient_cube(v, e, l_), direct_full(gridpp, g, o, v.astype(F32), e.astype(F32), l_.astype(F32), ds))
        same_bits(plan.simple_gradient_cube(v, 0.25), plan.simple_gradient_cube(v.astype(F32), 0.25))


def test_plan_outlives_its_grids():
    import gridpp_amd as gridpp
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        c = Case("warped", "grid", None, seed=21, Y=19, X=23)
        cube, ecube = c.cube(5, 2), c.cube(5, 3)
        want = [direct_full(gridpp, c.igrid, c.out, cube, ecube, c.lgrad, ds), direct_simple(gridpp, c.igrid, c.out, cube, 0.3, ds)]
        plan = gridpp.downscaling_plan(c.igrid, c.out, ds)
        lgrad = c.lgrad
        c.igrid = c.out = None
        del c
        gc.collect()
        same_bits(plan.full_gradient_cube(cube, ecube, lgrad), want[0])
        same_bits(plan.simple_gradient_cube(cube, 0.3), want[1])
        plan.release()
        for use in (lambda: plan.simple_gradient_cube(cube, 0.3), lambda: plan.full_gradient_cube(cube, ecube, lgrad)):
            with pytest.raises(RuntimeError, match="the plan was released"):
                use()
