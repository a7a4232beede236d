"""CPU-only: the two entries for the correlations of one point against many are declared in include/gridpp_hip.h, exported by the
library and bound in gridpp_amd/_capi.py with the argument types of their prototypes."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C parameter (as the header writes it) -> what _capi.py must declare for it
_structp = "const gpp_structure*"
EXPECTED = {
    "gpp_structure_corr_many": [(_structp, "struct"), ("const float p1[7]", "fp"), ("const float*", "vp"), ("long long", C.c_longlong),
                                ("int", C.c_int), ("float*", "vp")],
    "gpp_structure_corr_points": [(_structp, "struct"), ("const float p1[7]", "fp"), ("gpp_points*", "vp"), ("int", C.c_int),
                                  ("float*", "vp"), ("int", C.c_int)],
}


def _prototype(name):
    text = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in include/gridpp_hip.h" % name
    params = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        if not p.endswith("]"):
            p = re.sub(r"\s*\b[a-z_0-9]+$", "", p)   # drop the parameter's name
        params.append(p)
    return params


@pytest.fixture(scope="module")
def lib():
    from gridpp_amd import _capi
    return _capi.lib()


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_entry_is_declared_exported_and_bound(lib, name):
    from gridpp_amd import _capi
    kinds = {"struct": C.POINTER(_capi.gpp_structure), "fp": C.POINTER(C.c_float), "vp": C.c_void_p}
    assert _prototype(name) == [c for c, _ in EXPECTED[name]]
    assert _capi.SIGNATURES[name] == [kinds.get(k, k) for _, k in EXPECTED[name]]
    f = getattr(lib, name)
    f = getattr(f, "fn", f)   # (the suite wraps the entries)
    assert f.restype is C.c_int


def test_null_arguments_are_invalid_and_empty_input_is_ok(lib):
    """the argument checks come before anything touches a device"""
    from gridpp_amd import _capi
    import gridpp_amd as gridpp
    s = gridpp.BarnesStructure(1000)._s
    p1 = (C.c_float * 7)(0, 0, 0, 0, 0, 0, 0)
    out = (C.c_float * 1)()
    null_p1 = C.POINTER(C.c_float)()
    assert lib.gpp_structure_corr_many(None, p1, None, 0, 0, None) == _capi.GPP_EINVAL
    assert b"structure is NULL" in lib.gpp_last_error()
    assert lib.gpp_structure_corr_many(C.byref(s), null_p1, None, 0, 0, None) == _capi.GPP_EINVAL
    assert b"p1 is NULL" in lib.gpp_last_error()
    assert lib.gpp_structure_corr_many(C.byref(s), p1, None, 0, 0, None) == _capi.GPP_OK
    empty = gridpp.Points()
    assert lib.gpp_structure_corr_points(None, p1, empty._h, 0, out, 0) == _capi.GPP_EINVAL
    assert lib.gpp_structure_corr_points(C.byref(s), null_p1, empty._h, 0, out, 0) == _capi.GPP_EINVAL
    assert lib.gpp_structure_corr_points(C.byref(s), p1, empty._h, 0, out, 0) == _capi.GPP_OK
    assert gridpp.BarnesStructure(1000).corr(gridpp.Point(0, 0), []).shape == (0,)
    assert gridpp.BarnesStructure(1000).corr(gridpp.Point(0, 0), gridpp.Grid()).shape == (0, 0)
