"""CPU: the reusable OI gain through gridpp_amd and through the C-ABI without a GPU -- where its names live (gridpp_amd, not the alias
package; a header of its own, not gridpp.hpp), GPP_OI_GAIN_MAX_POINTS against its Python mirror, every ValueError and their order
before any device work, and "no HIP device" for a real build where no GPU is visible."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import __graft_entry__ as g
    g.build()
    import gridpp_amd
    return gridpp_amd


def small(amd, S=5):
    lats, lons = np.meshgrid(np.linspace(0, 1, 4), np.linspace(0, 1, 6), indexing="ij")
    grid = amd.Grid(lats, lons)
    points = amd.Points(np.linspace(0.1, 0.9, S), np.linspace(0.2, 0.8, S))
    return grid, points, np.full(S, 0.5, np.float32)


def test_names_live_in_gridpp_amd_only(amd):
    import gridpp
    assert gridpp.implementation == "gridpp_amd"
    assert not hasattr(gridpp, "optimal_interpolation_gain") and not hasattr(gridpp, "OiGain")
    assert callable(amd.optimal_interpolation_gain)
    for name in ("apply", "analysis_variance", "counts", "indices", "weights", "nbytes", "release"):
        assert hasattr(amd.OiGain, name)
    assert gridpp.optimal_interpolation is amd.optimal_interpolation


def test_cpp_class_has_a_header_of_its_own():
    own = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp_oi_gain.hpp")).read()
    assert re.search(r"class OiGain \{", own) and '#include "gridpp.hpp"' in own
    assert re.search(r"OiGain\(const Grid& bgrid, const Points& points, const vec& pratios, const StructureFunction& structure, int max_points", own)
    assert re.search(r"OiGain\(const Points& bpoints, const Points& points, const vec& pratios, const StructureFunction& structure, int max_points", own)
    for sig in (r"vec2 apply\(const vec2& background, const vec& pobs, const vec& pbackground, bool allow_extrapolation = true\) const",
                r"vec3 apply\(const vec3& background, const vec& pobs, const vec2& pbackground, bool allow_extrapolation = true\) const",
                r"vec apply\(const vec& background, const vec& pobs, const vec& pbackground, bool allow_extrapolation = true\) const",
                r"vec2 apply\(const vec2& background, const vec& pobs, const vec2& pbackground, bool allow_extrapolation = true\) const",
                r"vec2 analysis_variance\(const vec2& bvariance\) const", r"vec analysis_variance\(const vec& bvariance\) const"):
        assert re.search(sig, own), sig
    main = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    assert "OiGain" not in main and "oi_gain" not in main
    header = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    for entry in ("create", "apply", "variance", "info", "selection", "destroy"):
        assert re.search(r"int gpp_oi_gain_%s\(" % entry, header), entry


def test_constant_follows_the_header(amd):
    from gridpp_amd import _capi
    header = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    (value,) = re.findall(r"#define GPP_OI_GAIN_MAX_POINTS (\d+)", header)
    assert int(value) == _capi.OI_GAIN_MAX_POINTS >= 62
    for entry in ("create", "apply", "variance", "info", "selection", "destroy"):
        assert "gpp_oi_gain_" + entry in _capi.SIGNATURES


def test_value_errors_and_their_order(amd):
    """coordinate types, then max_points (0, -1, cap + 1), then the sizes of pratios and usable -- none of them needs a device"""
    from gridpp_amd import _capi
    grid, points, ratios = small(amd)
    st = amd.BarnesStructure(50000)
    cart = amd.Points([0.0, 1.0, 2.0, 3.0, 4.0], [0.0, 1.0, 2.0, 3.0, 4.0], (), (), amd.Cartesian)
    cap = _capi.OI_GAIN_MAX_POINTS
    # every later mistake is present as well: the first one is reported
    with pytest.raises(ValueError, match="same coordinate type"):
        amd.optimal_interpolation_gain(grid, cart, ratios[:2], st, 0, usable=[1])
    for mp in (0, -1):
        with pytest.raises(ValueError, match="max_points must be >= 1"):
            amd.optimal_interpolation_gain(grid, points, ratios[:2], st, mp, usable=[1])
    with pytest.raises(ValueError, match="max_points must be <= %d" % cap):
        amd.optimal_interpolation_gain(grid, points, ratios[:2], st, cap + 1, usable=[1])
    with pytest.raises(ValueError, match="Ratios .* size mismatch"):
        amd.optimal_interpolation_gain(grid, points, ratios[:2], st, cap, usable=[1])
    with pytest.raises(ValueError, match="usable .* size mismatch"):
        amd.optimal_interpolation_gain(grid, points, ratios, st, cap, usable=[1])
    with pytest.raises(TypeError):
        amd.optimal_interpolation_gain(ratios, points, ratios, st, 5)


def test_c_abi_checks_before_any_device_work(amd):
    from gridpp_amd import _capi
    lib = _capi.lib()
    grid, points, ratios = small(amd)
    cart = amd.Points([0.0, 1.0], [0.0, 1.0], (), (), amd.Cartesian)
    st = amd.BarnesStructure(50000)
    h = C.c_void_p()

    def create(g, p, mp):
        return lib.gpp_oi_gain_create(g, p, C.c_void_p(ratios.ctypes.data), None, C.byref(st._s), mp, C.byref(h))

    def status(rc, text):
        assert rc == _capi.GPP_EINVAL and text in lib.gpp_last_error().decode()

    status(create(grid._h, cart._h, 0), "Both background and observations points must be of same coordinate type (lat/lon or x/y)")
    status(create(grid._h, points._h, 0), "max_points must be >= 1")
    status(create(grid._h, points._h, -1), "max_points must be >= 1")
    status(create(grid._h, points._h, _capi.OI_GAIN_MAX_POINTS + 1), "GPP_OI_GAIN_MAX_POINTS")
    status(create(None, points._h, 5), "NULL")
    status(lib.gpp_oi_gain_apply(None, None, 1, None, 0, None, 1, None, 0), "NULL")
    status(lib.gpp_oi_gain_variance(None, None, None, 0), "NULL")
    status(lib.gpp_oi_gain_selection(None, None, None, None, 0), "NULL")
    status(lib.gpp_oi_gain_info(None, None, None, None, None, None), "NULL")
    assert lib.gpp_oi_gain_destroy(None) == _capi.GPP_OK
    assert h.value is None


def test_a_real_build_fails_loudly_without_a_gpu(amd):
    """no CPU path behind the gain: "no HIP device" where none is visible (where one is, the build simply works)"""
    grid, points, ratios = small(amd)
    st = amd.BarnesStructure(50000)
    if amd.device_count() > 0:
        gain = amd.optimal_interpolation_gain(grid, points, ratios, st, 3)
        assert gain.counts().shape == (4, 6) and gain.nbytes > 0
        gain.release()
        with pytest.raises(RuntimeError, match="released"):
            gain.counts()
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        amd.optimal_interpolation_gain(grid, points, ratios, st, 3)
