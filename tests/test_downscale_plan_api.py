"""CPU: the reusable downscaling plan through gridpp_amd and through the C-ABI without a GPU -- where its names live (gridpp_amd, not the
alias package; a header of its own, not gridpp.hpp), every entry point in the C header and in its Python mirror, every TypeError /
ValueError and their order before any device work, NULL handles, and "no HIP device" for a real build where no GPU is visible."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("create", "apply", "apply_cube", "simple_gradient", "full_gradient", "info", "destroy")


@pytest.fixture(scope="module")
def amd():
    import __graft_entry__ as g
    g.build()
    import gridpp_amd
    return gridpp_amd


def small(amd, ctype=None):
    lats, lons = np.meshgrid(np.linspace(0, 1, 4), np.linspace(0, 1, 6), indexing="ij")
    grid = amd.Grid(lats, lons, np.ones((4, 6)), np.ones((4, 6)))
    points = amd.Points(np.linspace(0.1, 0.9, 5), np.linspace(0.2, 0.8, 5), np.ones(5), np.ones(5), amd.Geodetic if ctype is None else ctype)
    return grid, points


def test_names_live_in_gridpp_amd_only(amd):
    import gridpp
    assert gridpp.implementation == "gridpp_amd"
    assert not hasattr(gridpp, "downscaling_plan") and not hasattr(gridpp, "DownscalingPlan")
    assert callable(amd.downscaling_plan)
    for name in ("apply", "apply_cube", "simple_gradient", "full_gradient", "nbytes", "distorted", "release"):
        assert hasattr(amd.DownscalingPlan, name)
    assert gridpp.downscaling is amd.downscaling and gridpp.full_gradient is amd.full_gradient


def test_cpp_class_has_a_header_of_its_own():
    own = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp_downscale_plan.hpp")).read()
    assert re.search(r"class DownscalingPlan \{", own) and '#include "gridpp.hpp"' in own
    assert re.search(r"DownscalingPlan\(const Grid& igrid, const Grid& ogrid, Downscaler downscaler", own)
    assert re.search(r"DownscalingPlan\(const Grid& igrid, const Points& opoints, Downscaler downscaler", own)
    for sig in (r"vec2 apply\(const vec2& ivalues\) const", r"vec3 apply\(const vec3& ivalues\) const", r"vec apply_points\(const vec2& ivalues\) const",
                r"vec2 apply_points\(const vec3& ivalues\) const", r"vec3 apply_cube\(const vec3& ivalues\) const",
                r"vec2 apply_cube_points\(const vec3& ivalues\) const", r"vec2 simple_gradient\(const vec2& ivalues, float elev_gradient\) const",
                r"vec2 full_gradient\(const vec2& ivalues, const vec2& elev_gradient, const vec2& laf_gradient = vec2\(\)\) const",
                r"long long nbytes\(\) const", r"~DownscalingPlan\(\)", r"DownscalingPlan\(const DownscalingPlan&\) = delete",
                r"DownscalingPlan& operator=\(const DownscalingPlan&\) = delete", r"DownscalingPlan\(DownscalingPlan&& o\) noexcept",
                r"DownscalingPlan& operator=\(DownscalingPlan&& o\) noexcept"):
        assert re.search(sig, own), sig
    main = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    assert "DownscalingPlan" not in main and "downscale_plan" not in main


def test_every_entry_point_is_declared_and_mirrored(amd):
    from gridpp_amd import _capi
    header = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    for entry in ENTRIES:
        assert re.search(r"int gpp_downscale_plan_%s\(" % entry, header), entry
        assert "gpp_downscale_plan_" + entry in _capi.SIGNATURES
        assert hasattr(_capi.lib(), "gpp_downscale_plan_" + entry)
    assert os.path.exists(os.path.join(ROOT, "gridpp_amd", "csrc", "downscale_plan.hip"))


def test_construction_errors_and_their_order(amd):
    """the two sets, then the downscaler, then (Nearest only) the coordinate types: the order of the direct call -- none needs a device"""
    grid, points = small(amd)
    _, cart = small(amd, amd.Cartesian)
    with pytest.raises(TypeError, match="the input must be a Grid"):
        amd.downscaling_plan(points, cart, 7)
    with pytest.raises(TypeError, match="the output must be a Grid or Points"):
        amd.downscaling_plan(grid, np.zeros(3), 7)
    # every later mistake is present as well: the first one is reported
    with pytest.raises(ValueError, match="Invalid downscaler"):
        amd.downscaling_plan(grid, cart, 7)
    with pytest.raises(ValueError, match="Coordinate types must be the same"):
        amd.downscaling_plan(grid, cart, amd.Nearest)
    with pytest.raises(ValueError, match="Coordinate types must be the same"):
        amd.downscaling_plan(grid, cart)   # Nearest is the default


@pytest.fixture
def fake_plan(amd, monkeypatch):
    """-> a factory of DownscalingPlans of the 4 x 6 grid with no plan of the library behind them, while no entry point of the library
    can be reached: the checks of the methods come before any device work"""
    def boom(*a, **k):
        raise AssertionError("the library was called")
    for entry in ENTRIES:
        monkeypatch.setattr(amd._capi.lib(), "gpp_downscale_plan_" + entry, boom, raising=False)
    made = []

    def make(output, downscaler, handle=1):
        grid, points = small(amd)
        made.append(amd.DownscalingPlan(handle, grid, grid if output == "grid" else points, downscaler))
        return made[-1]
    yield make
    for plan in made:   # (nothing to destroy: the entry points come back after this)
        plan._h = None


def test_method_errors_come_before_device_work(amd, fake_plan):
    ok, wrong = np.zeros((4, 6), np.float32), np.zeros((4, 5), np.float32)
    for out in ("grid", "points"):
        plan = fake_plan(out, amd.Bilinear)
        for call in (plan.apply, lambda v: plan.simple_gradient(v, 0.1), lambda v: plan.full_gradient(v, [], [])):
            with pytest.raises(RuntimeError, match="values must be 2-D or 3-D"):
                call(np.zeros(6, np.float32))
            with pytest.raises(ValueError, match="Grid size is not the same as values"):
                call(np.zeros((2, 4, 5), np.float32))
        with pytest.raises(ValueError, match="Grid size is not the same as values"):
            plan.apply(wrong)
        with pytest.raises(ValueError, match="Grid size is not the same as values"):
            plan.simple_gradient(wrong, 0.1)
        with pytest.raises(ValueError, match="Grid size is not the same as values"):
            plan.apply(np.zeros((2, 0, 6), np.float32))   # levels without rows pass the size rule, but there is nothing to read
        assert plan.apply(np.zeros((0, 4, 6), np.float32)).shape[0] == 0   # no level: an empty result, no call
        with pytest.raises(RuntimeError, match=r"apply_cube: values must be 3-D \(Y, X, E\)"):
            plan.apply_cube(ok)
        with pytest.raises(ValueError, match="Grid size is not the same as values"):
            plan.apply_cube(np.zeros((6, 4, 3), np.float32))
        assert plan.apply_cube(np.zeros((4, 6, 0), np.float32)).shape[-1] == 0   # no member: an empty result, no call
    # full_gradient: the overload rules and messages of the direct call, in its order
    grid_plan, points_plan = fake_plan("grid", amd.Nearest), fake_plan("points", amd.Nearest)
    with pytest.raises(ValueError, match="Values is the wrong size"):
        grid_plan.full_gradient(wrong, wrong)
    with pytest.raises(ValueError, match="Grid size is not the same as values"):
        points_plan.full_gradient(wrong, wrong, wrong)
    with pytest.raises(TypeError, match="laf_gradient is required"):
        points_plan.full_gradient(ok, ok)
    with pytest.raises(TypeError, match="laf_gradient is required"):
        grid_plan.full_gradient(np.zeros((2, 4, 6), np.float32), np.zeros((2, 4, 6), np.float32))
    with pytest.raises(ValueError, match="Laf gradient is the wrong size"):
        grid_plan.full_gradient(ok, wrong, wrong)   # the laf gradient is checked first
    with pytest.raises(ValueError, match="Elevation gradient is the wrong size"):
        grid_plan.full_gradient(ok, wrong, ok)
    with pytest.raises(ValueError, match="Elevation gradient is the wrong size"):
        grid_plan.full_gradient(ok, wrong)


def test_a_released_plan_raises(fake_plan):
    plan = fake_plan("grid", 0, handle=None)
    ok = np.zeros((4, 6), np.float32)
    for call in (lambda: plan.apply(ok), lambda: plan.apply_cube(np.zeros((4, 6, 2), np.float32)), lambda: plan.simple_gradient(ok, 0.0),
                 lambda: plan.full_gradient(ok, ok), lambda: plan.nbytes, lambda: plan.distorted):
        with pytest.raises(RuntimeError, match="the plan was released"):
            call()


def test_c_abi_checks_before_any_device_work(amd):
    from gridpp_amd import _capi
    lib = _capi.lib()
    grid, points = small(amd)
    _, cart = small(amd, amd.Cartesian)
    h = C.c_void_p()

    def status(rc, text):
        assert rc == _capi.GPP_EINVAL and text in lib.gpp_last_error().decode()

    status(lib.gpp_downscale_plan_create(None, points._h, 0, C.byref(h)), "NULL")
    status(lib.gpp_downscale_plan_create(grid._h, None, 0, C.byref(h)), "NULL")
    status(lib.gpp_downscale_plan_create(grid._h, points._h, 0, None), "NULL")
    status(lib.gpp_downscale_plan_create(points._h, grid._h, 7, C.byref(h)), "the input must be a Grid")
    status(lib.gpp_downscale_plan_create(grid._h, cart._h, 7, C.byref(h)), "Invalid downscaler")
    status(lib.gpp_downscale_plan_create(grid._h, cart._h, 0, C.byref(h)), "Coordinate types must be the same")
    status(lib.gpp_downscale_plan_apply(None, None, 1, None, 0), "NULL")
    status(lib.gpp_downscale_plan_apply_cube(None, None, 1, None, 0), "NULL")
    status(lib.gpp_downscale_plan_simple_gradient(None, None, 1, 0.0, None, 0), "NULL")
    status(lib.gpp_downscale_plan_full_gradient(None, None, 1, None, None, None, 0), "NULL")
    status(lib.gpp_downscale_plan_info(None, None, None, None, None, None), "NULL")
    assert lib.gpp_downscale_plan_destroy(None) == _capi.GPP_OK
    assert h.value is None


def test_a_real_build_fails_loudly_without_a_gpu(amd):
    """no CPU path behind the plan: "no HIP device" where none is visible (where one is, the build simply works)"""
    grid, points = small(amd)
    if amd.device_count() > 0:
        plan = amd.downscaling_plan(grid, points, amd.Bilinear)
        assert plan.apply(np.zeros((4, 6), np.float32)).shape == (5,) and plan.nbytes >= 16 * 5 and plan.distorted == 0
        plan.release()
        with pytest.raises(RuntimeError, match="released"):
            plan.apply(np.zeros((4, 6), np.float32))
        return
    for ds in (amd.Nearest, amd.Bilinear):
        with pytest.raises(RuntimeError, match="no HIP device"):
            amd.downscaling_plan(grid, points, ds)
