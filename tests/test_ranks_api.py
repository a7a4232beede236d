"""CPU: calc_ranks, sort_rows, reorder_by_ranks and calc_crps through `import gridpp_amd` without a GPU -- the four names and their
arguments, their absence from the `gridpp` alias and from gridpp.hpp, the header of their own, the three C-ABI declarations in gridpp_hip.h
with their bindings in _capi.py, every error and the order they come in (all before any device work), the empty shapes with their dtypes,
the C-ABI checks that need no device and "no HIP device" for a real call where no GPU is visible; and the numpy restatement the GPU tests
compare with (tests/rows_rank_ref.py) held to the counting definition of a rank and to the rank form of the CRPS."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests import rows_rank_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("calc_ranks", "sort_rows", "reorder_by_ranks", "calc_crps")
DIMS = "^array must have 1, 2 or 3 dimensions$"
SAME = "^reorder_by_ranks: values and template must have the same shape$"
REF = "^calc_crps: ref must have the shape of ensemble without its last axis$"
MIXED = "either all field arguments are torch CUDA tensors or none is"
DECLS = {
    "gpp_calc_ranks": ("int gpp_calc_ranks(const float* array, long rows, int len, int* ranks, float* sorted, int mem);",
                       [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "gpp_reorder_by_ranks": ("int gpp_reorder_by_ranks(const float* values, const float* templ, long rows, int len, float* out, int mem);",
                             [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int]),
    "gpp_calc_crps": ("int gpp_calc_crps(const float* ensemble, const float* ref, long rows, int len, float* out, int mem);",
                      [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int]),
}


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


class FakeDevice:   # what _marshal takes for a device tensor; the errors come before anything touches it
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape

    def data_ptr(self):
        return 0

    def dim(self):
        return len(self.shape)

    def contiguous(self):
        return self

    def to(self, dtype):
        return self


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_names_and_arguments(amd):
    assert list(inspect.signature(amd.calc_ranks).parameters) == ["array"]
    assert list(inspect.signature(amd.sort_rows).parameters) == ["array"]
    assert list(inspect.signature(amd.reorder_by_ranks).parameters) == ["values", "template"]
    assert list(inspect.signature(amd.calc_crps).parameters) == ["ensemble", "ref"]
    doc = amd.reorder_by_ranks.__doc__
    assert "ECC-Q" in doc and "Schaake shuffle" in doc and "broken by position" in doc and "not at random" in doc
    for name in NAMES:
        assert "DESIGN.md 4.18" in getattr(amd, name).__doc__, name


def test_the_alias_does_not_carry_them(amd):
    import gridpp
    assert gridpp.implementation == "gridpp_amd"
    for name in NAMES:
        assert callable(getattr(amd, name)) and not hasattr(gridpp, name), name
    assert gridpp.calc_quantile is amd.calc_quantile


def test_cpp_header_of_its_own():
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    for name in NAMES + ("gridpp_ranks",):
        assert name not in hpp, name
    own = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp_ranks.hpp")).read()
    for decl in ('#include "gridpp.hpp"', "inline ivec calc_ranks(const vec& array)", "inline ivec2 calc_ranks(const vec2& array)",
                 "inline ivec3 calc_ranks(const vec3& array)", "inline vec sort_rows(const vec& array)", "inline vec2 sort_rows(const vec2& array)",
                 "inline vec3 sort_rows(const vec3& array)", "inline vec reorder_by_ranks(const vec& values, const vec& templ)",
                 "inline vec2 reorder_by_ranks(const vec2& values, const vec2& templ)", "inline vec3 reorder_by_ranks(const vec3& values, const vec3& templ)",
                 "inline float calc_crps(const vec& ensemble, float ref)", "inline vec calc_crps(const vec2& ensemble, const vec& ref)",
                 "inline vec2 calc_crps(const vec3& ensemble, const vec2& ref)"):
        assert decl in own, decl
    for message in (SAME, REF):
        assert 'std::invalid_argument("%s")' % message[1:-1] in own, message


def test_c_abi_declarations_and_bindings(amd, lib):
    from gridpp_amd import _capi
    text = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    for name, (decl, sig) in DECLS.items():
        assert decl in text, name
        assert _capi.SIGNATURES[name] == sig, name
        assert callable(getattr(lib, name))
    assert "GPP_ROWS_RANKS" in text


# ---- errors, in their order, before any device work ---------------------------------------------------------------------------------------
def test_errors_and_their_order(amd):
    a = np.arange(12, dtype=F).reshape(3, 4)
    for wrong in (np.zeros((2, 2, 2, 2), F), np.zeros((1, 1, 1, 3, 4), F)):
        for call in (lambda: amd.calc_ranks(wrong), lambda: amd.sort_rows(wrong),
                     lambda: amd.reorder_by_ranks(wrong, a),                      # ... before the shapes are compared
                     lambda: amd.reorder_by_ranks(a, wrong), lambda: amd.calc_crps(wrong, a)):
            with pytest.raises(RuntimeError, match=DIMS):
                call()
    for other in (np.zeros((3, 5), F), np.zeros((4, 3), F), np.zeros(12, F), np.zeros((1, 3, 4), F)):
        with pytest.raises(ValueError, match=SAME):
            amd.reorder_by_ranks(a, other)
    for bad in (np.zeros(4, F), np.zeros((3, 4), F), np.zeros((3, 1), F), 1.0):
        with pytest.raises(ValueError, match=REF):
            amd.calc_crps(a, bad)
    with pytest.raises(ValueError, match=REF):
        amd.calc_crps(np.zeros((2, 3, 4), F), np.zeros((3, 2), F))
    # shapes before the memory kinds, the memory kinds before any device work
    with pytest.raises(ValueError, match=SAME):
        amd.reorder_by_ranks(a, FakeDevice(3, 5))
    with pytest.raises(ValueError, match=REF):
        amd.calc_crps(FakeDevice(3, 4), np.zeros(4, F))
    with pytest.raises(ValueError, match=MIXED):
        amd.reorder_by_ranks(a, FakeDevice(3, 4))
    with pytest.raises(ValueError, match=MIXED):
        amd.reorder_by_ranks(FakeDevice(3, 4), a)
    with pytest.raises(ValueError, match=MIXED):
        amd.calc_crps(a, FakeDevice(3))
    with pytest.raises(ValueError, match=MIXED):
        amd.calc_crps(FakeDevice(3, 4), np.zeros(3, F))


def test_empty_shapes_and_dtypes(amd):
    for shape in ((0,), (0, 4), (3, 0), (0, 3, 4), (2, 0, 4), (2, 3, 0)):
        a = np.zeros(shape, F)
        r, s, o = amd.calc_ranks(a), amd.sort_rows(a), amd.reorder_by_ranks(a, a)
        assert isinstance(r, np.ndarray) and r.dtype == np.int32 and r.shape == shape, shape
        assert s.dtype == F and s.shape == shape and o.dtype == F and o.shape == shape, shape
    for shape in ((0, 4), (0, 3, 4), (2, 0, 4)):
        c = amd.calc_crps(np.zeros(shape, F), np.zeros(shape[:-1], F))
        assert isinstance(c, np.ndarray) and c.dtype == F and c.shape == shape[:-1], shape
    with pytest.raises(ValueError, match=SAME):                                   # empty arrays do not hide a mismatch
        amd.reorder_by_ranks(np.zeros((0, 4), F), np.zeros((0, 5), F))


# ---- the C-ABI without a device ---------------------------------------------------------------------------------------------------------------
def test_c_abi_checks_before_device_work(lib):
    from gridpp_amd import _capi
    a, y = np.full((4, 8), 0.5, F), np.zeros(4, F)
    ranks, out, one = np.full((4, 8), 7, np.int32), np.full((4, 8), 7, F), np.full(4, 7, F)
    for call, good in ((lib.gpp_calc_ranks, (ptr(a), 4, 8, ptr(ranks), ptr(out), 0)),
                       (lib.gpp_reorder_by_ranks, (ptr(a), ptr(a), 4, 8, ptr(out), 0)),
                       (lib.gpp_calc_crps, (ptr(a), ptr(y), 4, 8, ptr(one), 0))):
        rows_at = 1 if call is lib.gpp_calc_ranks else 2
        for at in (rows_at, rows_at + 1):                                         # a negative size
            args = list(good)
            args[at] = -1
            assert call(*args) == _capi.GPP_EINVAL and "negative size" in lib.gpp_last_error().decode()
        args = list(good)
        args[rows_at] = 0                                                         # no rows: nothing to do, whatever the pointers
        assert call(*args) == _capi.GPP_OK
        assert call(*[None if isinstance(v, C.c_void_p) else v for v in args]) == _capi.GPP_OK
        for at, v in enumerate(good):                                             # a NULL pointer
            if not isinstance(v, C.c_void_p) or (call is lib.gpp_calc_ranks and at in (3, 4)):
                continue
            args = list(good)
            args[at] = None
            assert call(*args) == _capi.GPP_EINVAL and "NULL" in lib.gpp_last_error().decode(), at
    assert lib.gpp_calc_ranks(ptr(a), 4, 8, None, None, 0) == _capi.GPP_EINVAL    # either output may be NULL, not both
    assert "both NULL" in lib.gpp_last_error().decode()
    assert lib.gpp_calc_ranks(ptr(a), 4, 0, ptr(ranks), ptr(out), 0) == _capi.GPP_OK          # rows without a value: nothing to write
    assert lib.gpp_reorder_by_ranks(ptr(a), ptr(a), 4, 0, ptr(out), 0) == _capi.GPP_OK
    assert np.all(ranks == 7) and np.all(out == 7) and np.all(one == 7)           # nothing was written


def test_a_real_call_fails_loudly_without_a_gpu(amd, lib):
    """no CPU path behind the names: "no HIP device" where none is visible (where one is, the calls simply work)"""
    from gridpp_amd import _capi
    a = np.array([[3, 1, np.nan, 1], [0.0, -0.0, 2, -1]], F)
    if amd.device_count() > 0:
        assert amd.calc_ranks(a).tolist() == [[2, 0, -1, 1], [1, 2, 3, 0]]
        assert float(amd.calc_crps(a[0], 1.0)) == pytest.approx(2.0 / 9.0, rel=1e-6)
        return
    for call in (lambda: amd.calc_ranks(a), lambda: amd.sort_rows(a[0]), lambda: amd.reorder_by_ranks(a, a), lambda: amd.calc_crps(a, np.zeros(2, F)),
                 lambda: amd.calc_crps(np.zeros((2, 0), F), np.zeros(2, F))):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
    ranks, out = np.zeros((2, 4), np.int32), np.zeros((2, 4), F)
    assert lib.gpp_calc_ranks(ptr(a), 2, 4, ptr(ranks), None, 0) == _capi.GPP_ENODEVICE
    assert lib.gpp_calc_ranks(ptr(a), 2, 4, None, ptr(out), 0) == _capi.GPP_ENODEVICE
    assert lib.gpp_reorder_by_ranks(ptr(a), ptr(a), 2, 4, ptr(out), 0) == _capi.GPP_ENODEVICE
    assert lib.gpp_calc_crps(ptr(a), ptr(a), 2, 4, ptr(out), 0) == _capi.GPP_ENODEVICE


# ---- the restatement the GPU tests compare with ---------------------------------------------------------------------------------------------
def test_restatement_known_answers():
    nan = np.nan
    row = np.array([3, 1, nan, 1, np.inf, 0.0, -0.0], F)
    assert ref.ranks(row).tolist() == [4, 2, -1, 3, -1, 0, 1]
    s = ref.sorted_row(row)
    assert s[:5].tolist() == [0.0, 0.0, 1, 1, 3] and np.isnan(s[5:]).all()
    assert not np.signbit(s[0]) and np.signbit(s[1])                              # position decides between the zeros, the bits stay
    got = ref.reorder(np.array([10, nan, 30, 20], F), np.array([0.5, 0.1, 0.9, 0.7], F))
    assert got[[0, 1, 3]].tolist() == [20.0, 10.0, 30.0] and np.isnan(got[2])     # rank 3 >= the 3 valid values
    assert ref.crps_pairwise(np.array([1, 2, 3], F), 2.0) == pytest.approx(2 / 3 - 8 / 18)
    assert ref.crps_pairwise(np.array([5, nan], F), 7.0) == 2.0                   # N = 1: |x - y|
    assert np.isnan(ref.crps_pairwise(np.array([nan, np.inf], F), 0.0)) and np.isnan(ref.crps_pairwise(np.array([1, 2], F), np.inf))


def test_restatement_on_3000_random_rows():
    """argsort(kind="stable") on the valid values IS the counting definition, in every row; the pairwise CRPS and the rank form differ in
    float64 by at most 8 N 2^-53 (max |x| + |y|), in every row"""
    rng = np.random.default_rng(418)
    worst = 0.0
    for row, y in ref.random_rows(rng, 3000):
        np.testing.assert_array_equal(ref.ranks(row), ref.ranks_by_counting(row))
        a, b = ref.crps_pairwise(row, y), ref.crps_rank_form(row, y)
        if np.isnan(a) or np.isnan(b):
            assert np.isnan(a) and np.isnan(b)
            continue
        slack = ref.crps_slack(row, y)
        assert abs(a - b) <= slack, (row, y, a, b, slack)
        worst = max(worst, abs(a - b) / slack if slack else 0.0)
    print("largest |pairwise - rank form| / bound over 3000 rows: %.3f" % worst)
