"""CPU: neighbourhood_quantiles_fast and neighbourhood_cdf through `import gridpp_amd` without a GPU -- the two names and their arguments,
their absence from the `gridpp` alias and from gridpp.hpp, the header of their own (it compiles with the host compiler), the C-ABI
declarations and bindings, the errors of the two wrappers in their order (all before any device work), the empty shapes, the C-ABI checks
that need no device and "no HIP device" for a real call where no GPU is visible; and the yardstick of the GPU tests: the numpy restatement
of the reference's yarray (tests/nbh_cdf_ref.py) -> tests/curve_ref.interpolate gives the oracle's neighbourhood_quantile_fast
(DESIGN.md 4.17)."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import nbh_cdf_ref
from tests.test_gpu_neighbourhood_parity import close      # the project's measure: 1e-5 relative over a floor of 1e-3, NaN where the other is NaN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


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
    assert list(inspect.signature(amd.neighbourhood_quantiles_fast).parameters) == ["input", "quantiles", "halfwidth", "thresholds"]
    assert list(inspect.signature(amd.neighbourhood_cdf).parameters) == ["input", "thresholds", "halfwidth"]
    assert "1 - cdf" in amd.neighbourhood_cdf.__doc__ and "DESIGN.md 4.17" in amd.neighbourhood_cdf.__doc__
    assert "DESIGN.md 4.17" in amd.neighbourhood_quantiles_fast.__doc__


def test_the_alias_does_not_carry_them(amd):
    """neither has a counterpart in the reference: a script asks for them by gridpp_amd's name"""
    import gridpp
    assert gridpp.implementation == "gridpp_amd"
    assert callable(amd.neighbourhood_quantiles_fast) and callable(amd.neighbourhood_cdf)
    assert not hasattr(gridpp, "neighbourhood_quantiles_fast") and not hasattr(gridpp, "neighbourhood_cdf")
    assert gridpp.neighbourhood_quantile_fast is amd.neighbourhood_quantile_fast


def test_cpp_header_of_its_own(tmp_path):
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    assert "neighbourhood_quantiles_fast" not in hpp and "neighbourhood_cdf" not in hpp and "gridpp_nbh_quantiles" not in hpp
    own = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp_nbh_quantiles.hpp")).read()
    for decl in ('#include "gridpp.hpp"',
                 "inline vec3 neighbourhood_quantiles_fast(const vec2& input, const vec& quantiles, int halfwidth, const vec& thresholds)",
                 "inline vec3 neighbourhood_quantiles_fast(const vec3& input, const vec& quantiles, int halfwidth, const vec& thresholds)",
                 "inline vec3 neighbourhood_cdf(const vec2& input, const vec& thresholds, int halfwidth)",
                 "inline vec3 neighbourhood_cdf(const vec3& input, const vec& thresholds, int halfwidth)",
                 "inline void neighbourhood_quantiles_fast_device(", "inline void neighbourhood_cdf_device(",
                 'std::invalid_argument("Half width must be > 0")'):
        assert decl in own, decl
    # the header and the program the GPU test drives compile with the host compiler: the two headers only, no library, no GPU
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "gridpp_amd", "host"),
           os.path.join(ROOT, "tests", "cpp", "test_nbh_quantiles.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_c_abi_declarations_and_bindings(amd, lib):
    from gridpp_amd import _capi
    text = " ".join(open(os.path.join(ROOT, "include", "gridpp_hip.h")).read().split())
    for decl in ("int gpp_neighbourhood_quantiles_fast(const float* input, int ny, int nx, int ne, int is3d, const float* quantiles, int nq, "
                 "int halfwidth, const float* thresholds, int nt, float* out, int mem);",
                 "int gpp_neighbourhood_cdf(const float* input, int ny, int nx, int ne, int is3d, int halfwidth, const float* thresholds, int nt, "
                 "float* out, int mem);"):
        assert decl in text, decl
    vp, i = C.c_void_p, C.c_int
    assert _capi.SIGNATURES["gpp_neighbourhood_quantiles_fast"] == [vp, i, i, i, i, vp, i, i, vp, i, vp, i]
    assert _capi.SIGNATURES["gpp_neighbourhood_cdf"] == [vp, i, i, i, i, i, vp, i, vp, i]
    assert callable(lib.gpp_neighbourhood_quantiles_fast) and callable(lib.gpp_neighbourhood_cdf)


# ---- errors, in their order, before any device work ---------------------------------------------------------------------------------------
def test_errors_and_their_order(amd):
    f, thr = np.zeros((4, 5, 3), F), [0.0, 1.0]
    with pytest.raises(ValueError, match="^Half width must be > 0$"):
        amd.neighbourhood_quantiles_fast(f, [1.5], -1, thr)                                 # ... before the level's range
    with pytest.raises(ValueError, match="^Half width must be > 0$"):
        amd.neighbourhood_quantiles_fast(np.zeros((0, 5, 3), F), [0.5], -1, thr)            # ... and before the empty field
    with pytest.raises(ValueError, match="^Half width must be > 0$"):
        amd.neighbourhood_cdf(f, thr, -1)
    with pytest.raises(ValueError, match="^Half width must be > 0$"):
        amd.neighbourhood_cdf(np.zeros((0, 0), F), thr, -2)
    for bad in ([0.5, 1.5], [-0.1], [np.nan, 2.0], [0.2, 0.4, 1.0000001]):
        with pytest.raises(ValueError, match="^All quantiles must be >= 0 and <= 1$"):
            amd.neighbourhood_quantiles_fast(f, bad, 1, thr)
        with pytest.raises(ValueError, match="^All quantiles must be >= 0 and <= 1$"):
            amd.neighbourhood_quantiles_fast(f[:, :, 0], bad, 1, thr)
        with pytest.raises(ValueError, match="^All quantiles must be >= 0 and <= 1$"):
            amd.neighbourhood_quantiles_fast(f, bad, 1, [])                                 # no thresholds do not hide a bad level
    with pytest.raises(RuntimeError, match="quantiles must have 1 dimensions"):               # no per-cell level fields here
        amd.neighbourhood_quantiles_fast(f, np.full((4, 5), 0.5, F), 1, thr)
    for wrong in (np.zeros(4, F), np.zeros((2, 2, 2, 2), F)):
        with pytest.raises(RuntimeError, match="^input must have 2 or 3 dimensions$"):
            amd.neighbourhood_quantiles_fast(wrong, [0.5], 1, thr)
        with pytest.raises(RuntimeError, match="^input must have 2 or 3 dimensions$"):
            amd.neighbourhood_cdf(wrong, thr, 1)


def test_empty_shapes(amd):
    f = np.zeros((4, 5, 3), F)
    for empty in (np.zeros((0, 5, 3), F), np.zeros((4, 0, 3), F), np.zeros((4, 5, 0), F), np.zeros((0, 0), F), [[]]):
        for out in (amd.neighbourhood_quantiles_fast(empty, [0.5, 0.9], 1, [0.0, 1.0]), amd.neighbourhood_cdf(empty, [0.0, 1.0], 1),
                    amd.neighbourhood_quantiles_fast(empty, [1.5], 1, [0.0, 1.0])):       # (an empty field comes before the levels, as in the single-level call)
            assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == (0, 0, 0)
    for g in (f, f[:, :, 0]):
        out = amd.neighbourhood_quantiles_fast(g, [], 1, [0.0, 1.0])                        # no levels
        assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == (4, 5, 0)
        out = amd.neighbourhood_cdf(g, [], 1)                                               # no thresholds
        assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == (4, 5, 0)


# ---- the C-ABI without a device ---------------------------------------------------------------------------------------------------------------
def test_c_abi_checks_before_device_work(lib):
    from gridpp_amd import _capi
    f, q, thr = np.full((4, 5, 3), 0.5, F), np.array([0.25, 0.75], F), np.array([0.0, 1.0], F)
    out = np.full((4, 5, 2), 7, F)
    levels, cdf = lib.gpp_neighbourhood_quantiles_fast, lib.gpp_neighbourhood_cdf

    def message():
        return lib.gpp_last_error().decode()
    assert levels(ptr(f), 4, 5, 3, 1, ptr(q), 2, -1, ptr(thr), 2, ptr(out), 0) == _capi.GPP_EINVAL and message() == "Half width must be > 0"
    assert cdf(ptr(f), 4, 5, 3, 1, -1, ptr(thr), 2, ptr(out), 0) == _capi.GPP_EINVAL and message() == "Half width must be > 0"
    assert levels(None, 4, 5, 3, 1, None, 2, -1, None, 2, None, 0) == _capi.GPP_EINVAL and message() == "Half width must be > 0"   # first of all
    for args in ((None, 4, 5, 3, 1, ptr(q), 2, 1, ptr(thr), 2, ptr(out), 0), (ptr(f), 4, 5, 3, 1, None, 2, 1, ptr(thr), 2, ptr(out), 0),
                 (ptr(f), 4, 5, 3, 1, ptr(q), 2, 1, None, 2, ptr(out), 0), (ptr(f), 4, 5, 3, 1, ptr(q), 2, 1, ptr(thr), 2, None, 0)):
        assert levels(*args) == _capi.GPP_EINVAL and "NULL" in message()
    for args in ((None, 4, 5, 3, 1, 1, ptr(thr), 2, ptr(out), 0), (ptr(f), 4, 5, 3, 1, 1, None, 2, ptr(out), 0), (ptr(f), 4, 5, 3, 1, 1, ptr(thr), 2, None, 0)):
        assert cdf(*args) == _capi.GPP_EINVAL and "NULL" in message()
    for level in (1.5, -0.25):
        bad = np.array([0.5, level], F)
        assert levels(ptr(f), 4, 5, 3, 1, ptr(bad), 2, 1, ptr(thr), 2, ptr(out), 0) == _capi.GPP_EINVAL
        assert message() == "All quantiles must be >= 0 and <= 1"
    assert levels(ptr(f), 4, 5, 3, 1, ptr(q), -1, 1, ptr(thr), 2, ptr(out), 0) == _capi.GPP_EINVAL
    assert levels(ptr(f), 4, 5, 3, 1, ptr(q), 2, 1, ptr(thr), -1, ptr(out), 0) == _capi.GPP_EINVAL
    assert cdf(ptr(f), 4, 5, 3, 1, 1, ptr(thr), -1, ptr(out), 0) == _capi.GPP_EINVAL
    # nothing to compute: an empty field, no levels, no thresholds for the cdf
    assert levels(ptr(f), 0, 5, 3, 1, ptr(q), 2, 1, ptr(thr), 2, ptr(out), 0) == _capi.GPP_OK
    assert levels(None, 4, 0, 3, 1, None, 2, 1, None, 2, None, 0) == _capi.GPP_OK
    assert levels(ptr(f), 4, 5, 3, 1, ptr(q), 0, 1, ptr(thr), 2, ptr(out), 0) == _capi.GPP_OK
    assert levels(ptr(f), 4, 5, 3, 1, None, 0, 1, ptr(thr), 2, None, 0) == _capi.GPP_OK
    assert cdf(ptr(f), 4, 5, 0, 1, 1, ptr(thr), 2, ptr(out), 0) == _capi.GPP_OK
    assert cdf(ptr(f), 4, 5, 3, 1, 1, None, 0, None, 0) == _capi.GPP_OK
    assert np.all(out == 7)                                                                  # nothing was written


def test_a_real_call_fails_loudly_without_a_gpu(amd, lib):
    """no CPU path behind the names: "no HIP device" where none is visible (where one is, the call simply works)"""
    from gridpp_amd import _capi
    f = np.arange(60, dtype=F).reshape(4, 5, 3)
    thr = np.array([10.0, 30.0, 50.0], F)
    if amd.device_count() > 0:
        assert amd.neighbourhood_quantiles_fast(f, [0.0, 1.0], 1, thr).shape == (4, 5, 2) and amd.neighbourhood_cdf(f, thr, 1).shape == (4, 5, 3)
        return
    for call in (lambda: amd.neighbourhood_quantiles_fast(f, [0.5, 0.9], 1, thr), lambda: amd.neighbourhood_quantiles_fast(f[:, :, 0], [0.5], 1, thr),
                 lambda: amd.neighbourhood_quantiles_fast(f, [0.5, np.nan], 1, []), lambda: amd.neighbourhood_cdf(f, thr, 1),
                 lambda: amd.neighbourhood_cdf(f[:, :, 0], thr, 20)):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
    q, out = np.array([0.5, np.nan], F), np.zeros((4, 5, 3), F)                               # (a NaN level passes the range check)
    assert lib.gpp_neighbourhood_quantiles_fast(ptr(f), 4, 5, 3, 1, ptr(q), 2, 1, ptr(thr), 3, ptr(out), 0) == _capi.GPP_ENODEVICE
    assert lib.gpp_neighbourhood_cdf(ptr(f), 4, 5, 3, 1, 1, ptr(thr), 3, ptr(out), 0) == _capi.GPP_ENODEVICE


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------------
def case_12x9x5():
    rng = np.random.default_rng(1209)
    f = rng.uniform(0, 10, (12, 9, 5)).astype(F)
    f[rng.random(f.shape) < 0.08] = np.nan
    f[0, 0, 1] = np.inf
    f[3:8, 2:7, :] = np.nan            # with halfwidth 1 the windows of (4..6, 3..5) hold no valid cell
    return f


@pytest.mark.parametrize("hw", [0, 1, 3])
def test_restatement_chain_gives_the_oracles_quantile_fast(hw):
    """fractions -> the oracle's Mean -> E-fold float32 sum / E -> clamp -> interpolate (+ the two special cases) against the oracle's own
    neighbourhood_quantile_fast on a 12 x 9 x 5 cube and on its first member as a 2-D field: thresholds sorted, permuted and with a duplicate,
    levels at both ends, on a threshold's expected rank and NaN."""
    from oracle import oracle as O
    f = case_12x9x5()
    rng = np.random.default_rng(5)
    sorted_thr = np.linspace(0, 10, 6).astype(F)
    dup = sorted_thr.copy()
    dup[2] = dup[3]
    for field in (f, f[:, :, 0].copy()):
        for thr in (sorted_thr, rng.permutation(sorted_thr), dup, np.array([5.0], F), np.array([-1.0, 11.0], F)):
            ya = nbh_cdf_ref.cdf(O, field, thr, hw)
            assert ya.shape == field.shape[:2] + (thr.size,) and ya.dtype == F
            ok = ~np.isnan(ya)
            assert (ya[ok] >= 0).all() and (ya[ok] <= 1).all()
            assert (np.isnan(ya).any(axis=2) == np.isnan(ya).all(axis=2)).all()           # a window without a valid cell has none for any threshold
            empty = np.isnan(O.neighbourhood(nbh_cdf_ref.fractions(field, thr[0]), hw, O.Mean))
            assert (np.isnan(ya[:, :, 0]) == empty).all()
            if hw == 1 and field.ndim == 3:
                assert empty[5, 4] and not empty[0, 0]
            for q in (0.0, 0.1, 0.5, 0.9, 1.0, np.nan):
                close(nbh_cdf_ref.quantile_from_cdf(ya, thr, q), O.neighbourhood_quantile_fast(field, [q], hw, thr))


def test_restatement_known_answers():
    """small cases by hand: one cell, one member -- the fraction is 0 or 1, the fold keeps it, and the special cases take the ends"""
    class Same:          # a stand-in for the oracle where the window is the cell itself
        Mean = 0

        @staticmethod
        def neighbourhood(plane, hw, stat):
            return plane
    ya = nbh_cdf_ref.cdf(Same, np.array([[[1.0, 2.0, 3.0, np.nan]]], F), [0.0, 1.0, 2.5, 3.0, np.inf], 0)
    third = nbh_cdf_ref.fold(np.array([F(1) / F(3)], F), 4)[0]
    two_thirds = nbh_cdf_ref.fold(np.array([F(2) / F(3)], F), 4)[0]
    assert ya.tolist() == [[[0.0, third, two_thirds, 1.0, 1.0]]]
    assert abs(float(third) - 1 / 3) < 1e-6 and abs(float(two_thirds) - 2 / 3) < 1e-6
    assert np.isnan(nbh_cdf_ref.cdf(Same, np.full((1, 1, 3), np.nan, F), [1.0], 0)).all()
    thr = np.array([0.0, 1.0, 2.5, 3.0], F)
    assert nbh_cdf_ref.quantile_from_cdf(ya[:, :, :4], thr, 1.0)[0, 0] == 3.0
    assert nbh_cdf_ref.quantile_from_cdf(ya[:, :, :4], thr, 0.0)[0, 0] == 0.0
    assert np.isnan(nbh_cdf_ref.quantile_from_cdf(ya[:, :, :4], thr, np.nan)[0, 0])
    assert nbh_cdf_ref.quantile_from_cdf(np.zeros((1, 1, 2), F), [4.0, 6.0], 0.0)[0, 0] == 6.0      # :516-517: quantile 0 and nothing below the last threshold
    assert nbh_cdf_ref.quantile_from_cdf(np.ones((1, 1, 2), F), [4.0, 6.0], 1.0)[0, 0] == 4.0       # :514-515
