"""CPU: the cube-layout gradients and the planned ensemble downscalers of gridpp_amd.DownscalingPlan without a GPU -- where the names
live (on the plan of gridpp_amd and of gridpp_downscale_plan.hpp, nowhere else), the four new entry points in the C header and its
Python mirror, every error and its order before any device work (the fake plans of tests/test_downscale_plan_api.py), NULL handles
and negative member counts through the C-ABI, a released plan, and "no HIP device" for a real build where no GPU is visible."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("simple_gradient_cube", "full_gradient_cube", "probability", "mask_threshold")
ALL_ENTRIES = ("create", "apply", "apply_cube", "simple_gradient", "full_gradient", "info", "destroy") + NEW_ENTRIES
METHODS = ("simple_gradient_cube", "full_gradient_cube", "downscale_probability", "mask_threshold_downscale_consensus",
           "mask_threshold_downscale_quantile")
Y, X, E = 4, 6, 3


@pytest.fixture(scope="module")
def amd():
    import __graft_entry__ as g
    g.build()
    import gridpp_amd
    return gridpp_amd


def small(amd, ctype=None):
    lats, lons = np.meshgrid(np.linspace(0, 1, Y), np.linspace(0, 1, X), indexing="ij")
    ctype = amd.Geodetic if ctype is None else ctype
    grid = amd.Grid(lats, lons, np.ones((Y, X)), np.ones((Y, X)), type=ctype)
    points = amd.Points(np.linspace(0.1, 0.9, 5), np.linspace(0.2, 0.8, 5), np.ones(5), np.ones(5), ctype)
    return grid, points


def test_names_live_on_the_plan_only(amd):
    import gridpp
    assert gridpp.implementation == "gridpp_amd"
    assert not hasattr(gridpp, "downscaling_plan") and not hasattr(gridpp, "DownscalingPlan")
    for name in METHODS:
        assert callable(getattr(amd.DownscalingPlan, name)), name
    for name in ("simple_gradient_cube", "full_gradient_cube"):   # no top-level name, in either package
        assert not hasattr(amd, name) and not hasattr(gridpp, name)
    assert gridpp.downscale_probability is amd.downscale_probability   # the direct calls stay what they were


def test_every_new_entry_point_is_declared_bound_and_exported(amd):
    from gridpp_amd import _capi
    header = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    for entry in NEW_ENTRIES:
        assert re.search(r"int gpp_downscale_plan_%s\(" % entry, header), entry
        assert "gpp_downscale_plan_" + entry in _capi.SIGNATURES
        assert hasattr(_capi.lib(), "gpp_downscale_plan_" + entry)
    assert re.search(r"int gpp_downscale_plan_full_gradient_cube\(gpp_downscale_plan\* plan, const float\* values, int ne, const float\* elev_gradient,\s*"
                     r"int elev_members,\s*const float\* laf_gradient, int laf_members, float\* out, int mem\)", header)
    assert os.path.exists(os.path.join(ROOT, "gridpp_amd", "csrc", "ensemble_downscale.h"))


def test_cpp_header_carries_the_new_methods():
    own = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp_downscale_plan.hpp")).read()
    for sig in (r"vec3 simple_gradient_cube\(const vec3& ivalues, float elev_gradient\) const",
                r"vec2 simple_gradient_cube_points\(const vec3& ivalues, float elev_gradient\) const",
                r"vec3 full_gradient_cube\(const vec3& ivalues, const EG& elev_gradient, const LG& laf_gradient\) const",
                r"vec2 full_gradient_cube_points\(const vec3& ivalues, const EG& elev_gradient, const LG& laf_gradient\) const",
                r"cube_gradient\(const vec2& g,", r"cube_gradient\(const vec3& g,",
                r"vec2 downscale_probability\(const vec3& ivalues, const vec2& threshold, const ComparisonOperator& comparison_operator\) const",
                r"vec2 mask_threshold_downscale_consensus\(const vec3& ivalues_true, const vec3& ivalues_false, const vec3& threshold_values, "
                r"const vec2& threshold,\s*const ComparisonOperator& comparison_operator, const Statistic& statistic\) const",
                r"vec2 mask_threshold_downscale_quantile\(const vec3& ivalues_true, const vec3& ivalues_false, const vec3& threshold_values, "
                r"const vec2& threshold,\s*const ComparisonOperator& comparison_operator, const float quantile_level\) const"):
        assert re.search(sig, own), sig
    main = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    assert "DownscalingPlan" not in main and "downscale_plan" not in main


@pytest.fixture
def fake_plan(amd, monkeypatch):
    """-> a factory of DownscalingPlans of the 4 x 6 grid with no plan of the library behind them, while no entry point of the library
    can be reached (the approach of tests/test_downscale_plan_api.py)"""
    def boom(*a, **k):
        raise AssertionError("the library was called")
    for entry in ALL_ENTRIES:
        monkeypatch.setattr(amd._capi.lib(), "gpp_downscale_plan_" + entry, boom, raising=False)
    made = []

    def make(output, downscaler, handle=1, otype=None):
        grid, points = small(amd)
        ogrid, opoints = small(amd, otype)
        made.append(amd.DownscalingPlan(handle, grid, ogrid if output == "grid" else opoints, downscaler))
        return made[-1]
    yield make
    for plan in made:
        plan._h = None


def test_gradient_cube_errors_come_before_device_work(amd, fake_plan):
    cube = np.zeros((Y, X, E), np.float32)
    ok2 = np.zeros((Y, X), np.float32)
    for out in ("grid", "points"):
        plan = fake_plan(out, amd.Bilinear)
        for name, call in (("simple_gradient_cube", lambda v: plan.simple_gradient_cube(v, 0.1)),
                           ("full_gradient_cube", lambda v: plan.full_gradient_cube(v, ok2, ok2))):
            with pytest.raises(RuntimeError, match=r"%s: values must be 3-D \(Y, X, E\)" % name):
                call(ok2)
            with pytest.raises(ValueError, match="Grid size is not the same as values"):
                call(np.zeros((X, Y, E), np.float32))
            assert call(np.zeros((Y, X, 0), np.float32)).shape == plan._oshape + (0,)   # no member: an empty result, no call
        # the values come first, then the laf gradient, then the elevation gradient
        with pytest.raises(ValueError, match="Grid size is not the same as values"):
            plan.full_gradient_cube(np.zeros((Y, X + 1, E), np.float32), np.zeros((1, 1)), np.zeros((1, 1)))
        with pytest.raises(ValueError, match="Laf gradient is the wrong size"):
            plan.full_gradient_cube(cube, np.zeros((Y, X + 1)), np.zeros((Y, X + 1)))
        with pytest.raises(ValueError, match="Laf gradient is the wrong size"):
            plan.full_gradient_cube(cube, ok2, np.zeros((Y, X, E + 1)))    # a cube of another member count
        with pytest.raises(ValueError, match="Laf gradient is the wrong size"):
            plan.full_gradient_cube(cube, ok2, np.zeros((E, Y, X)))        # levels first is the other layout
        with pytest.raises(ValueError, match="Elevation gradient is the wrong size"):
            plan.full_gradient_cube(cube, np.zeros((Y, X, E + 1)), ok2)
        with pytest.raises(ValueError, match="Elevation gradient is the wrong size"):
            plan.full_gradient_cube(cube, np.zeros((Y, X + 1)), [])
        with pytest.raises(ValueError, match="Elevation gradient is the wrong size"):
            plan.full_gradient_cube(cube, np.zeros(Y * X), None)
        with pytest.raises(TypeError):
            plan.full_gradient_cube(cube, ok2)   # both gradients are required arguments
        # every accepted form reaches the library, and only then
        for eg, lg in ((ok2, ok2), (cube, cube), (ok2, cube), (cube, ok2), ([], ok2), (cube, None), ([], []), (None, None)):
            with pytest.raises(AssertionError, match="the library was called"):
                plan.full_gradient_cube(cube, eg, lg)
        with pytest.raises(AssertionError, match="the library was called"):
            plan.simple_gradient_cube(cube, 0.1)


def test_ensemble_errors_come_in_the_order_of_the_direct_calls(amd, fake_plan):
    cube, wrong = np.zeros((Y, X, E), np.float32), np.zeros((Y, X + 1, E), np.float32)
    th = np.zeros((Y, X), np.float32)   # (the fake output grid has the input's shape)
    for ds in (amd.Nearest, amd.Bilinear):
        plan = fake_plan("grid", ds)
        calls = {"downscale_probability": lambda c, t, op: plan.downscale_probability(c, t, op),
                 "mask_threshold_downscale_consensus": lambda c, t, op: plan.mask_threshold_downscale_consensus(c, c, c, t, op, amd.Mean),
                 "mask_threshold_downscale_quantile": lambda c, t, op: plan.mask_threshold_downscale_quantile(c, c, c, t, op, 0.5)}
        points_plan = fake_plan("points", ds)
        for name, call in calls.items():
            # a Points plan is refused first, whatever else is wrong
            with pytest.raises(TypeError, match="%s: the plan's output must be a Grid" % name):
                getattr(points_plan, name)(*([wrong] * (1 if name == "downscale_probability" else 3)), np.zeros(3), 7,
                                           *(() if name == "downscale_probability" else (0.5,)))
            # then the ranks, the grid size, the threshold, the operator -- each with every later mistake present as well
            with pytest.raises(RuntimeError, match="values must have 3 dimensions"):
                call(th, np.zeros(3), 7)
            with pytest.raises(RuntimeError, match="threshold must have 2 dimensions"):
                call(wrong, np.zeros(3), 7)
            with pytest.raises(ValueError, match="Grid size is not the same as values"):
                call(wrong, np.zeros((Y, X + 2), np.float32), 7)
            with pytest.raises(ValueError, match="Grid size is not the same as threshold"):
                call(cube, np.zeros((Y, X + 2), np.float32), 7)
            with pytest.raises(ValueError, match="Invalid comparison operator"):
                call(cube, th, 7)
            with pytest.raises(AssertionError, match="the library was called"):
                call(cube, th, amd.Gt)
        for name in ("mask_threshold_downscale_consensus", "mask_threshold_downscale_quantile"):
            with pytest.raises(ValueError, match="%s: ivalues_true, ivalues_false and threshold_values must have the same shape" % name):
                getattr(plan, name)(cube, wrong, cube, np.zeros((Y, X + 2), np.float32), 7, 99)
        with pytest.raises(ValueError, match="Invalid comparison operator"):
            plan.mask_threshold_downscale_consensus(cube, cube, cube, th, 7, 99)       # the operator before the statistic
        with pytest.raises(RuntimeError, match="Internal error. Cannot compute statistic"):
            plan.mask_threshold_downscale_consensus(cube, cube, cube, th, amd.Lt, 99)
        for q in (-0.1, 1.5):
            with pytest.raises(ValueError, match="calc_quantile: Quantile must be between 0 and 1 inclusive"):
                plan.mask_threshold_downscale_quantile(cube, cube, cube, th, amd.Lt, q)
    # a Bilinear plan may span two coordinate types (a Nearest one cannot be built); the ensemble downscalers refuse it, after the shapes
    across = fake_plan("grid", amd.Bilinear, otype=amd.Cartesian)
    with pytest.raises(ValueError, match="Grid size is not the same as threshold"):
        across.downscale_probability(cube, np.zeros((Y, X + 2), np.float32), 7)
    with pytest.raises(ValueError, match="Coordinate types must be the same"):
        across.downscale_probability(cube, th, 7)
    with pytest.raises(ValueError, match="Coordinate types must be the same"):
        across.mask_threshold_downscale_quantile(cube, cube, cube, th, 7, 3.0)
    with pytest.raises(AssertionError, match="the library was called"):
        across.full_gradient_cube(cube, th, th)   # the gradients do not mind


def test_a_released_plan_raises(fake_plan, amd):
    plan = fake_plan("grid", 0, handle=None)
    cube, th = np.zeros((Y, X, E), np.float32), np.zeros((Y, X), np.float32)
    for call in (lambda: plan.simple_gradient_cube(cube, 0.0), lambda: plan.full_gradient_cube(cube, th, th),
                 lambda: plan.downscale_probability(cube, th, amd.Gt),
                 lambda: plan.mask_threshold_downscale_consensus(cube, cube, cube, th, amd.Gt, amd.Mean),
                 lambda: plan.mask_threshold_downscale_quantile(cube, cube, cube, th, amd.Gt, 0.5)):
        with pytest.raises(RuntimeError, match="the plan was released"):
            call()


def test_c_abi_null_handles_and_negative_member_counts(amd):
    """statuses that need neither a device nor a plan: a NULL handle comes first, whatever else is wrong"""
    from gridpp_amd import _capi
    lib = _capi.lib()

    def status(rc, text):
        assert rc == _capi.GPP_EINVAL and text in lib.gpp_last_error().decode()

    for ne in (1, -1):
        status(lib.gpp_downscale_plan_simple_gradient_cube(None, None, ne, 0.0, None, 0), "plan handle is NULL")
        status(lib.gpp_downscale_plan_full_gradient_cube(None, None, ne, None, 1, None, 1, None, 0), "plan handle is NULL")
        status(lib.gpp_downscale_plan_probability(None, None, ne, None, 7, None, 0), "plan handle is NULL")
        status(lib.gpp_downscale_plan_mask_threshold(None, None, None, None, ne, None, 7, 99, 2.0, None, 0), "plan handle is NULL")
    if amd.device_count() == 0:
        return
    # with a device: a negative ne on a real plan, before anything is read
    grid, _ = small(amd)
    plan = amd.downscaling_plan(grid, grid, amd.Bilinear)
    status(lib.gpp_downscale_plan_simple_gradient_cube(plan._h, None, -1, 0.0, None, 0), "negative number of members")
    status(lib.gpp_downscale_plan_full_gradient_cube(plan._h, None, -1, None, 1, None, 1, None, 0), "negative number of members")
    status(lib.gpp_downscale_plan_probability(plan._h, None, -1, None, 0, None, 0), "negative number of ensemble members")
    status(lib.gpp_downscale_plan_mask_threshold(plan._h, None, None, None, -1, None, 0, 0, 0.0, None, 0), "negative number of ensemble members")
    th = np.zeros((Y, X), np.float32)
    status(lib.gpp_downscale_plan_full_gradient_cube(plan._h, th.ctypes.data_as(C.c_void_p), 4, th.ctypes.data_as(C.c_void_p), 3, None, 1,
                                                     th.ctypes.data_as(C.c_void_p), 0), "1 or ne members")
    assert lib.gpp_downscale_plan_simple_gradient_cube(plan._h, None, 0, 0.0, None, 0) == _capi.GPP_OK   # no member: nothing to do


def test_a_real_build_fails_loudly_without_a_gpu(amd):
    """no CPU path behind the new methods: a chain that ends in one of them gives "no HIP device" where none is visible (where one is,
    it simply works)"""
    grid, points = small(amd)
    cube, th = np.zeros((Y, X, E), np.float32), np.zeros((Y, X), np.float32)
    chains = [lambda ds: amd.downscaling_plan(grid, points, ds).simple_gradient_cube(cube, 0.5),
              lambda ds: amd.downscaling_plan(grid, grid, ds).full_gradient_cube(cube, th, cube),
              lambda ds: amd.downscaling_plan(grid, grid, ds).downscale_probability(cube, th, amd.Gt),
              lambda ds: amd.downscaling_plan(grid, grid, ds).mask_threshold_downscale_consensus(cube, cube, cube, th, amd.Gt, amd.Mean),
              lambda ds: amd.downscaling_plan(grid, grid, ds).mask_threshold_downscale_quantile(cube, cube, cube, th, amd.Gt, 0.5)]
    shapes = [(5, E), (Y, X, E), (Y, X), (Y, X), (Y, X)]
    for ds in (amd.Nearest, amd.Bilinear):
        for chain, shape in zip(chains, shapes):
            if amd.device_count() > 0:
                assert chain(ds).shape == shape
            else:
                with pytest.raises(RuntimeError, match="no HIP device"):
                    chain(ds)
