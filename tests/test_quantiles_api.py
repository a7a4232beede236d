"""CPU: calc_quantiles and quantile_mapping_curves through `import gridpp_amd` without a GPU -- the two names and their arguments, their
absence from the `gridpp` alias and from gridpp.hpp, the header of their own, the exported C-ABI symbol with its declaration in gridpp_hip.h
and its binding in _capi.py, every error of the two wrappers and the order they come in (all before any device work), the empty shapes, the
C-ABI checks that need no device (NULL, a level out of range, nq == 0 and rows == 0) and "no HIP device" for a real call where no GPU is
visible."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
RANGE = "^calc_quantiles: Quantiles must be between 0 and 1 inclusive$"


@pytest.fixture(scope="module")
def amd():
    import __graft_entry__ as g
    g.build()
    import gridpp_amd
    return gridpp_amd


@pytest.fixture(scope="module")
def lib(amd):
    from gridpp_amd import _capi
    return _capi.lib()


def ptr(a):
    return C.c_void_p(a.ctypes.data)


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_names_and_arguments(amd):
    assert list(inspect.signature(amd.calc_quantiles).parameters) == ["array", "quantiles"]
    assert list(inspect.signature(amd.quantile_mapping_curves).parameters) == ["ref", "fcst", "quantiles"]
    doc = amd.quantile_mapping_curves.__doc__
    assert "quantile_mapping.cpp:41-42" in doc and "TRUE quantiles" in doc and "quantile_mapping_curve" in doc
    assert "DESIGN.md 4.16" in amd.calc_quantiles.__doc__


def test_the_alias_does_not_carry_them(amd):
    """neither has a counterpart in the reference: a script asks for them by gridpp_amd's name"""
    import gridpp
    assert gridpp.implementation == "gridpp_amd"
    assert callable(amd.calc_quantiles) and callable(amd.quantile_mapping_curves)      # gridpp_amd has them: the alias pops them
    assert not hasattr(gridpp, "calc_quantiles") and not hasattr(gridpp, "quantile_mapping_curves")
    assert gridpp.calc_quantile is amd.calc_quantile and gridpp.quantile_mapping_curve is amd.quantile_mapping_curve


def test_cpp_header_of_its_own():
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    assert "calc_quantiles" not in hpp and "quantile_mapping_curves" not in hpp and "gridpp_quantiles" not in hpp
    own = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp_quantiles.hpp")).read()
    for decl in ('#include "gridpp.hpp"', "inline vec calc_quantiles(const vec& array, const vec& quantiles)",
                 "inline vec2 calc_quantiles(const vec2& array, const vec& quantiles)", "inline vec3 calc_quantiles(const vec3& array, const vec& quantiles)",
                 "inline vec3 quantile_mapping_curves(const vec3& ref, const vec3& fcst, vec3& output_fcst, const vec& quantiles)"):
        assert decl in own, decl
    for message in ("calc_quantiles: Quantiles must be between 0 and 1 inclusive", "Quantiles must be >= 0 and <= 1",
                    "quantile_mapping_curves: ref and fcst must have the same first two dimensions",
                    "quantile_mapping_curves: empty quantiles: the sorted-rows form is not built"):
        assert 'std::invalid_argument("%s")' % message in own, message


def test_c_abi_symbol_declaration_and_binding(amd, lib):
    from gridpp_amd import _capi
    text = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    decl = "int gpp_calc_quantiles(const float* array, long rows, int len, const float* quantiles, int nq, float* out, int mem);"
    assert decl in text
    comment = text[:text.index(decl)].rsplit("/*", 1)[1]
    assert "*/" in comment and comment.index("*/") > len(comment) - 8   # the comment directly above the declaration
    for word in ("[rows][nq]", "host", "GPP_EINVAL", "NaN passes", "GPP_ROWS_QUANTILES"):
        assert word in comment, word
    assert _capi.SIGNATURES["gpp_calc_quantiles"] == [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    assert callable(lib.gpp_calc_quantiles)


# ---- errors, in their order, before any device work ---------------------------------------------------------------------------------------
def test_calc_quantiles_errors(amd):
    a = np.arange(12, dtype=F).reshape(3, 4)
    for bad in ([0.5, 1.5], [-0.1], [np.nan, 2.0]):
        with pytest.raises(ValueError, match=RANGE):
            amd.calc_quantiles(a, bad)
    for wrong in (np.zeros((2, 2, 2, 2), F), np.zeros((1, 1, 1, 1, 4), F)):
        with pytest.raises(RuntimeError, match="^array must have 1, 2 or 3 dimensions$"):   # calc_quantile's wording
            amd.calc_quantiles(wrong, [0.5])
        with pytest.raises(RuntimeError, match="^array must have 1, 2 or 3 dimensions$"):   # ... and it comes before the range check
            amd.calc_quantiles(wrong, [1.5])
    with pytest.raises(RuntimeError, match="quantiles must have 1 dimensions"):
        amd.calc_quantiles(a, [[0.5, 0.6]])
    with pytest.raises(RuntimeError, match="quantiles must have 1 dimensions"):               # the shape of the levels before their range
        amd.calc_quantiles(a, [[0.5, 1.6]])


def test_calc_quantiles_empty_shapes(amd):
    for shape, q, want in (((3, 4), [], (3, 0)), ((0, 4), [0.1, 0.9], (0, 2)), ((4,), [], (0,)), ((2, 3, 4), [], (2, 3, 0)), ((0, 3, 4), [0.5], (0, 3, 1)),
                           ((2, 0, 4), [0.5, 0.6], (2, 0, 2))):
        out = amd.calc_quantiles(np.zeros(shape, F), q)
        assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == want, (shape, q)
    with pytest.raises(ValueError, match=RANGE):                                             # an empty array does not hide a bad level
        amd.calc_quantiles(np.zeros((0, 4), F), [1.5])


def test_quantile_mapping_curves_errors_and_their_order(amd):
    ref, fcst = np.zeros((2, 3, 5), F), np.zeros((2, 3, 4), F)
    for other in (np.zeros((2, 4, 4), F), np.zeros((3, 3, 4), F)):
        with pytest.raises(ValueError, match="^quantile_mapping_curves: ref and fcst must have the same first two dimensions$"):
            amd.quantile_mapping_curves(ref, other, [])                                     # ... before the empty levels
    with pytest.raises(ValueError, match="^quantile_mapping_curves: empty quantiles: the sorted-rows form is not built$"):
        amd.quantile_mapping_curves(ref, fcst, [])
    with pytest.raises(ValueError, match="^quantile_mapping_curves: empty quantiles"):
        amd.quantile_mapping_curves(ref, fcst, ())
    for bad in ([0.5, np.nan], [1.5], [-0.01, 0.5]):
        with pytest.raises(ValueError, match="^Quantiles must be >= 0 and <= 1$"):           # the reference's wording; NaN too
            amd.quantile_mapping_curves(ref, fcst, bad)
    for wrong in (np.zeros((2, 3), F), np.zeros(4, F)):
        with pytest.raises(RuntimeError, match="must have 3 dimensions"):
            amd.quantile_mapping_curves(wrong, fcst, [0.5])
        with pytest.raises(RuntimeError, match="must have 3 dimensions"):
            amd.quantile_mapping_curves(ref, wrong, [0.5])
    a, b = amd.quantile_mapping_curves(np.zeros((0, 3, 5), F), np.zeros((0, 3, 4), F), [0.1, 0.9])   # no cells: nothing to compute
    assert a.shape == (0, 3, 2) and b.shape == (0, 3, 2) and a.dtype == F


def test_mixed_host_and_device_inputs(amd):
    class FakeDevice:   # what _marshal takes for a device tensor; the error comes before anything touches it
        is_cuda = True
        shape = (2, 3, 4)

        def data_ptr(self):
            return 0

        def dim(self):
            return 3

        def contiguous(self):
            return self

        def to(self, dtype):
            return self

    with pytest.raises(ValueError, match="either all field arguments are torch CUDA tensors or none is"):
        amd.quantile_mapping_curves(np.zeros((2, 3, 5), F), FakeDevice(), [0.5])
    with pytest.raises(ValueError, match="either all field arguments"):                       # ... before the levels are looked at
        amd.quantile_mapping_curves(FakeDevice(), np.zeros((2, 3, 5), F), [])


# ---- the C-ABI without a device ---------------------------------------------------------------------------------------------------------------
def test_c_abi_checks_before_device_work(lib):
    from gridpp_amd import _capi
    a, q, out = np.full((4, 8), 0.5, F), np.array([0.25, 0.75], F), np.full((4, 2), 7, F)
    call = lib.gpp_calc_quantiles
    for args in ((None, 4, 8, ptr(q), 2, ptr(out), 0), (ptr(a), 4, 8, None, 2, ptr(out), 0), (ptr(a), 4, 8, ptr(q), 2, None, 0)):
        assert call(*args) == _capi.GPP_EINVAL and "NULL" in lib.gpp_last_error().decode()
    for level in (1.5, -0.25):
        bad = np.array([0.5, level], F)
        assert call(ptr(a), 4, 8, ptr(bad), 2, ptr(out), 0) == _capi.GPP_EINVAL
        assert lib.gpp_last_error().decode() == "calc_quantiles: Quantiles must be between 0 and 1 inclusive"
        assert call(ptr(a), 0, 8, ptr(bad), 2, ptr(out), 0) == _capi.GPP_EINVAL               # ... also with nothing to compute
    assert call(ptr(a), 4, 8, ptr(q), 0, ptr(out), 0) == _capi.GPP_OK
    assert call(ptr(a), 4, 8, None, 0, None, 0) == _capi.GPP_OK
    assert call(ptr(a), 0, 8, ptr(q), 2, ptr(out), 0) == _capi.GPP_OK
    assert call(None, 0, 8, ptr(q), 2, None, 0) == _capi.GPP_OK
    assert call(ptr(a), -1, 8, ptr(q), 2, ptr(out), 0) == _capi.GPP_EINVAL
    assert call(ptr(a), 4, 8, ptr(q), -1, ptr(out), 0) == _capi.GPP_EINVAL
    assert np.all(out == 7)                                                                  # nothing was written


def test_a_real_call_fails_loudly_without_a_gpu(amd, lib):
    """no CPU path behind the names: "no HIP device" where none is visible (where one is, the call simply works)"""
    from gridpp_amd import _capi
    a = np.arange(24, dtype=F).reshape(2, 3, 4)
    if amd.device_count() > 0:
        assert amd.calc_quantiles(a[0, 0], [0.5, 0.0]).tolist() == [1.5, 0.0]
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        amd.calc_quantiles(a, [0.5])
    with pytest.raises(RuntimeError, match="no HIP device"):
        amd.quantile_mapping_curves(a, a, [0.5])
    q, out = np.array([0.5, np.nan], F), np.zeros((6, 2), F)                                  # (a NaN level passes the range check)
    assert lib.gpp_calc_quantiles(ptr(a), 6, 4, ptr(q), 2, ptr(out), 0) == _capi.GPP_ENODEVICE
