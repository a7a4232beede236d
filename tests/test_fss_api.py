"""CPU: fractions_skill_score through `import gridpp_amd` without a GPU -- the name, its arguments and default, the named tuple, its absence
from the `gridpp` alias and from gridpp.hpp, the header of its own, the C-ABI declaration in gridpp_hip.h with its binding in _capi.py,
every error and the order they come in (all before any device work), the shapes that need no device, the C-ABI checks that need none and
"no HIP device" for a real call where no GPU is visible; and the numpy restatement the GPU tests compare with (tests/fss_ref.py) held to
hand-worked answers, to the composition users write today (the oracle's neighbourhood Mean of 0/1 float32 planes) and to the summation
bound the GPU tests use."""
import ctypes as C
import inspect
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import fss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MIXED = "either all field arguments are torch CUDA tensors or none is"
REF = "^fractions_skill_score: ref must have the shape \\(Y, X\\) of fcst$"
DECL = ("int gpp_fractions_skill_score(const float* fcst, const float* ref, int ny, int nx, int ne, int is3d, const float* thresholds, int nt,\n"
        "                              const int* halfwidths, int nh, int comparison_operator, double* fbs, double* fbs_worst, long long* cells, int mem);")
SIG = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
       C.c_void_p, C.c_int]


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
def test_name_arguments_and_result(amd):
    sig = inspect.signature(amd.fractions_skill_score)
    assert list(sig.parameters) == ["fcst", "ref", "thresholds", "halfwidths", "comparison_operator"]
    assert sig.parameters["comparison_operator"].default == amd.Gt == 20
    assert amd.FssResult._fields == ("fss", "fbs", "fbs_worst", "cells")
    doc = amd.fractions_skill_score.__doc__
    for words in ("DESIGN.md 4.22", "1 - sum(fbs) / sum(fbs_worst)", "POOLED member fraction", "bit-identical from call to call"):
        assert words in doc, words


def test_the_alias_does_not_carry_it(amd):
    import gridpp
    assert gridpp.implementation == "gridpp_amd"
    for name in ("fractions_skill_score", "FssResult"):
        assert hasattr(amd, name) and not hasattr(gridpp, name), name
    assert gridpp.neighbourhood_score is amd.neighbourhood_score
    assert "fractions_skill_score" in open(os.path.join(ROOT, "gridpp", "__init__.py")).read()   # the comment there says why


def test_cpp_header_of_its_own():
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    for name in ("fractions_skill_score", "FssResult", "gridpp_fss"):
        assert name not in hpp, name
    own = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp_fss.hpp")).read()
    for decl in ('#include "gridpp.hpp"', "struct FssResult {",
                 "inline FssResult fractions_skill_score(const vec2& fcst, const vec2& ref, const vec& thresholds, const ivec& halfwidths,\n"
                 "                                       ComparisonOperator comparison_operator = Gt)",
                 "inline FssResult fractions_skill_score(const vec3& fcst, const vec2& ref, const vec& thresholds, const ivec& halfwidths,\n"
                 "                                       ComparisonOperator comparison_operator = Gt)",
                 "GPP_FSS_VALUE("):
        assert decl in own, decl
    for message in ("fractions_skill_score: ref must have the shape (Y, X) of fcst", "fractions_skill_score: a threshold is NaN",
                    "Half width must be > 0", "Invalid comparison operator"):
        assert 'std::invalid_argument("%s")' % message in own, message


def test_c_abi_declaration_and_binding(amd, lib):
    from gridpp_amd import _capi
    text = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    assert DECL in text
    assert _capi.SIGNATURES["gpp_fractions_skill_score"] == SIG
    assert callable(lib.gpp_fractions_skill_score)
    assert "#define GPP_FSS_VALUE(fbs, fbs_worst)" in text and "GPP_FSS_GENERAL" in text and "GPP_FSS_FILL" in text
    for name, v in (("TILE_COLS", _capi.FSS_TILE_COLS), ("TILE_ROWS", _capi.FSS_TILE_ROWS), ("FUSED_MAXHW", _capi.FSS_FUSED_MAXHW)):
        assert "#define GPP_FSS_%s %d " % (name, v) in text, name


# ---- errors, in their order, before any device work ---------------------------------------------------------------------------------------
def test_errors_and_their_order(amd):
    f, r = np.zeros((3, 4), F), np.zeros((3, 4), F)
    nan = math.nan
    fss = amd.fractions_skill_score
    # 1. the number of dimensions, before everything else
    for wrong in (np.zeros(5, F), np.zeros((2, 2, 2, 2), F)):
        with pytest.raises(RuntimeError, match="fcst must have 2 or 3 dimensions"):
            fss(wrong, np.zeros((9, 9), F), [[nan]], [-1], 99)
    for wrong in (np.zeros(12, F), np.zeros((3, 4, 1), F)):
        with pytest.raises(RuntimeError, match="ref must have 2 dimensions"):
            fss(f, wrong, [[nan]], [-1], 99)
    with pytest.raises(RuntimeError, match="ref must have 2 dimensions"):
        fss(FakeDevice(3, 4), FakeDevice(3, 4, 1), [0.5], [1])
    # 2. the shape of ref
    for other in (np.zeros((4, 3), F), np.zeros((3, 5), F), np.zeros((0, 0), F)):
        with pytest.raises(ValueError, match=REF):
            fss(f, other, [[nan]], [-1], 99)
        with pytest.raises(ValueError, match=REF):
            fss(np.zeros((3, 4, 7), F), other, [0.5], [1])
    with pytest.raises(ValueError, match=REF):
        fss(f, FakeDevice(4, 3), [nan], [-1], 99)                   # ... before the memory kinds
    # 3. thresholds and halfwidths are 1-D
    for bad in (0.5, [[0.5]], np.zeros((2, 2))):
        with pytest.raises(ValueError, match="^fractions_skill_score: thresholds must have 1 dimension$"):
            fss(f, r, bad, [-1], 99)
    for bad in (1, [[1]], np.zeros((2, 2), int)):
        with pytest.raises(ValueError, match="^fractions_skill_score: halfwidths must have 1 dimension$"):
            fss(f, r, [nan], bad, 99)
    # 4. a NaN threshold; +-Inf are legal
    with pytest.raises(ValueError, match="^fractions_skill_score: a threshold is NaN$"):
        fss(f, r, [0.5, nan], [-1], 99)
    # 5. a half width that is no integer, or negative
    for bad in ([1.0], [0.5, 2], ["1"]):
        with pytest.raises(ValueError, match="^fractions_skill_score: halfwidths must be integers$"):
            fss(f, r, [0.5], bad, 99)
    with pytest.raises(ValueError, match="^Half width must be > 0$"):
        fss(f, r, [math.inf, -math.inf], [1, -1], 99)
    # 6. the operator
    for op in (99, 5, -1, None):
        with pytest.raises(ValueError, match="^Invalid comparison operator$"):
            fss(f, FakeDevice(3, 4), [0.5], [1], op)
    # 7. the memory kinds
    for a, b in ((f, FakeDevice(3, 4)), (FakeDevice(3, 4), r), (FakeDevice(3, 4, 5), r)):
        with pytest.raises(ValueError, match=MIXED):
            fss(a, b, [0.5], [1])
        with pytest.raises(ValueError, match=MIXED):
            fss(a, b, [], [])                                         # ... before the shapes that need no device


def test_shapes_that_need_no_device(amd):
    f, r = np.ones((3, 4), F), np.ones((3, 4), F)
    for thr, hws in (([], [1, 2]), ([0.5], []), ([], []), (np.zeros(0), np.zeros(0, int))):
        res = amd.fractions_skill_score(f, r, thr, hws)
        T, H = len(thr), len(hws)
        assert isinstance(res, amd.FssResult)
        for a in (res.fss, res.fbs, res.fbs_worst):
            assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (T, H)
        assert res.cells.dtype == np.int64 and res.cells.shape == (H,) and not res.cells.any()
    for fe, re in ((np.zeros((0, 0), F), np.zeros((0, 0), F)), ([[]], [[]]), (np.zeros((0, 5), F), np.zeros((0, 5), F)),
                   (np.zeros((3, 0), F), np.zeros((3, 0), F)), (np.zeros((3, 4, 0), F), r), (np.zeros((0, 4, 6), F), np.zeros((0, 4), F))):
        res = amd.fractions_skill_score(fe, re, [0.5, 1.5], [0, 1, 2], amd.Leq)
        assert res.fss.shape == (2, 3) and np.isnan(res.fss).all()
        assert res.fbs.dtype == np.float64 and not res.fbs.any() and not res.fbs_worst.any() and res.fbs_worst.shape == (2, 3)
        assert res.cells.dtype == np.int64 and res.cells.tolist() == [0, 0, 0]


# ---- the C-ABI without a device ---------------------------------------------------------------------------------------------------------------
def test_c_abi_checks_before_device_work(lib):
    from gridpp_amd import _capi
    f, r = np.zeros((3, 4), F), np.zeros((3, 4), F)
    thr, hws = np.array([0.5, 1.5], F), np.array([0, 1, 2], np.int32)
    fbs, worst, cells = np.full((2, 3), 7.0), np.full((2, 3), 7.0), np.full(3, 7, np.int64)
    good = [ptr(f), ptr(r), 3, 4, 1, 0, ptr(thr), 2, ptr(hws), 3, 20, ptr(fbs), ptr(worst), ptr(cells), 0]
    call = lib.gpp_fractions_skill_score
    for at in (2, 3, 4, 7, 9):                                       # a negative size
        args = list(good)
        args[at] = -1
        assert call(*args) == _capi.GPP_EINVAL and "negative size" in lib.gpp_last_error().decode(), at
    args = list(good)
    args[4] = 2                                                       # a 2-D forecast with members
    assert call(*args) == _capi.GPP_EINVAL and "ne == 1" in lib.gpp_last_error().decode()
    for at in (6, 8, 11, 12, 13):                                    # a NULL array that would be read or written
        args = list(good)
        args[at] = None
        assert call(*args) == _capi.GPP_EINVAL and "NULL" in lib.gpp_last_error().decode(), at
    bad = np.array([0.5, np.nan], F)
    assert call(*(good[:6] + [ptr(bad)] + good[7:])) == _capi.GPP_EINVAL and "threshold is NaN" in lib.gpp_last_error().decode()
    neg = np.array([0, -1, 2], np.int32)
    assert call(*(good[:8] + [ptr(neg)] + good[9:])) == _capi.GPP_EINVAL and lib.gpp_last_error().decode() == "Half width must be > 0"
    for op in (5, -1, 40):
        assert call(*(good[:10] + [op] + good[11:])) == _capi.GPP_EINVAL and lib.gpp_last_error().decode() == "Invalid comparison operator"
    assert (fbs == 7).all() and (worst == 7).all() and (cells == 7).all()                    # nothing was written
    # nothing to do: no device needed, the outputs that exist are zero
    args = list(good)
    args[7] = 0
    assert call(*args) == _capi.GPP_OK and (cells == 0).all() and (fbs == 7).all()
    cells[:] = 7
    args = list(good)
    args[2] = 0
    args[0] = args[1] = None
    assert call(*args) == _capi.GPP_OK and (cells == 0).all() and (fbs == 0).all() and (worst == 0).all()
    args = list(good)
    args[9] = 0
    args[8] = args[11] = args[12] = args[13] = None
    assert call(*args) == _capi.GPP_OK


def test_a_real_call_fails_loudly_without_a_gpu(amd, lib):
    """no CPU path behind the name: "no HIP device" where none is visible (where one is, the call simply works)"""
    from gridpp_amd import _capi
    f, r = np.zeros((3, 3), F), np.zeros((3, 3), F)
    f[0, 0] = r[2, 2] = 1
    if amd.device_count() > 0:
        res = amd.fractions_skill_score(f, r, [0.5], [0, 2])
        assert res.fss.tolist() == [[0.0, 1.0]] and res.cells.tolist() == [9, 9]
        return
    for call in (lambda: amd.fractions_skill_score(f, r, [0.5], [0, 2]), lambda: amd.fractions_skill_score(np.zeros((3, 3, 5)), r, [0.5], [300], amd.Lt)):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
    thr, hws = np.array([0.5], F), np.array([1], np.int32)
    fbs, worst, cells = np.zeros(1), np.zeros(1), np.zeros(1, np.int64)
    assert lib.gpp_fractions_skill_score(ptr(f), ptr(r), 3, 3, 1, 0, ptr(thr), 1, ptr(hws), 1, 20, ptr(fbs), ptr(worst), ptr(cells), 0) == _capi.GPP_ENODEVICE


# ---- the restatement the GPU tests compare with ---------------------------------------------------------------------------------------------
def by_hand(fcst, ref, threshold, h):
    """the definition once more, cell by cell in exact rationals (2-D, Gt) -> fbs, fbs_worst, cells"""
    Y, X = fcst.shape
    counts = np.isfinite(fcst) & np.isfinite(ref)
    fbs = worst = Fraction(0)
    cells = 0
    for y in range(Y):
        for x in range(X):
            n = K = O = 0
            for yy in range(max(y - h, 0), min(y + h, Y - 1) + 1):
                for xx in range(max(x - h, 0), min(x + h, X - 1) + 1):
                    if counts[yy, xx]:
                        n += 1
                        K += bool(fcst[yy, xx] > threshold)
                        O += bool(ref[yy, xx] > threshold)
            if n:
                Ff, Fo = Fraction(K, n), Fraction(O, n)
                fbs += (Ff - Fo) ** 2
                worst += Ff ** 2 + Fo ** 2
                cells += 1
    return fbs, worst, cells


def close(got, want, ulps=4):
    want = float(want)
    return abs(got - want) <= ulps * math.ulp(want)


def test_restatement_hand_worked_answers():
    f, r = np.zeros((3, 3), F), np.zeros((3, 3), F)
    f[0, 0] = r[2, 2] = 1
    res = R.fss(f, r, [0.5], [0, 1, 2])
    assert res.cells.tolist() == [9, 9, 9]
    assert res.fbs[0, 0] == 2 and res.fbs_worst[0, 0] == 2 and res.fss[0, 0] == 0
    assert close(res.fbs[0, 1], Fraction(17, 72)) and close(res.fbs_worst[0, 1], Fraction(169, 648)) and close(res.fss[0, 1], Fraction(16, 169), 16)
    assert res.fbs[0, 2] == 0 and close(res.fbs_worst[0, 2], Fraction(2, 9)) and res.fss[0, 2] == 1
    for h in (0, 1, 2):
        assert by_hand(f, r, 0.5, h) == ({0: 2, 1: Fraction(17, 72), 2: 0}[h], {0: 2, 1: Fraction(169, 648), 2: Fraction(2, 9)}[h], 9)
    r[1, 1] = np.nan                                                  # the centre does not count, yet contributes wherever a neighbour counts
    res = R.fss(f, r, [0.5], [0, 1, 2])
    for j, h in enumerate((0, 1, 2)):
        fbs, worst, cells = by_hand(f, r, 0.5, h)
        assert res.cells[j] == cells == (8 if h == 0 else 9)
        assert close(res.fbs[0, j], fbs) and close(res.fbs_worst[0, j], worst) and close(res.fss[0, j], 1 - fbs / worst, 16)
    # no event in either field: NaN; the operators at a tie
    assert np.isnan(R.fss(f, r, [5.0], [1]).fss[0, 0])
    k, m, o, c = R.cell_integers(f, r, 1.0, R.Geq)
    assert k.sum() == 1 and o.sum() == 1 and m.sum() == c.sum() == 8
    k, m, o, c = R.cell_integers(f, r, 1.0, R.Gt)
    assert k.sum() == 0 and o.sum() == 0
    assert R.cell_integers(f, r, 1.0, R.Lt)[0].sum() == 7 and R.cell_integers(f, r, 1.0, R.Leq)[0].sum() == 8


def composition_case():
    rng = np.random.default_rng(422)
    Y, X = 67, 131
    yy, xx = np.meshgrid(np.arange(Y), np.arange(X), indexing="ij")
    smooth = np.sin(yy / 9.0) + np.cos(xx / 13.0)
    f = (smooth + rng.normal(0, 0.5, (Y, X))).astype(F)
    r = (smooth + rng.normal(0, 0.5, (Y, X))).astype(F)
    for a in (f, r):
        bad = rng.random((Y, X)) < 0.03
        a[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(bad.sum()))
    r[20:45, 50:90] = np.nan                                          # a block wider than the small windows
    return f, r


THRESHOLDS = (-1.0, 0.0, 0.7, 1.6)
HALFWIDTHS = (0, 1, 2, 16, 17, 200)


def test_restatement_against_the_composition():
    """what users compose today: 0/1 float32 planes, NaN where a cell does not count, two neighbourhood Means, the sums in float64"""
    from oracle import oracle as O
    f, r = composition_case()
    counts = np.isfinite(f) & np.isfinite(r)
    res = R.fss(f, r, THRESHOLDS, HALFWIDTHS)
    worst_diff = 0.0
    for t, th in enumerate(THRESHOLDS):
        pf = np.where(counts, (f > F(th)).astype(F), F(np.nan)).astype(F)
        po = np.where(counts, (r > F(th)).astype(F), F(np.nan)).astype(F)
        for j, h in enumerate(HALFWIDTHS):
            mf, mo = O.neighbourhood(pf, h, O.Mean).astype(np.float64), O.neighbourhood(po, h, O.Mean).astype(np.float64)
            on = ~np.isnan(mf)
            assert (on == ~np.isnan(mo)).all()
            N = int(on.sum())
            assert N == res.cells[j]
            fbs, worst = float(((mf[on] - mo[on]) ** 2).sum()), float((mf[on] ** 2 + mo[on] ** 2).sum())
            diff = abs(R.value(fbs, worst) - res.fss[t, j])
            assert diff <= 2.0 ** -22 + (2 * N + 16) * 2.0 ** -53, (th, h, diff)
            worst_diff = max(worst_diff, diff)
    print("largest |fss - composition| over %d pairs: %.3g" % (len(THRESHOLDS) * len(HALFWIDTHS), worst_diff))


def test_summation_bound_of_the_gpu_tests():
    """N terms of one sign: float64 additions in any order stay within (N - 1) 2^-53 of the exact sum, relative (every addition rounds a
    partial sum that is at most the total), and math.fsum is within 2^-53 of it: (N + 8) 2^-53 covers both.  Forward and reversed running
    sums on the composition case are held to it; the share of the bound they use is printed (0.17 at most here)"""
    f, r = composition_case()
    share = 0.0
    for th in THRESHOLDS:
        for h in HALFWIDTHS:
            for terms in R.terms(f, r, th, h):
                total, N = math.fsum(terms), terms.size
                assert (terms >= 0).all() and total > 0
                for order in (terms, terms[::-1]):
                    err = abs(float(np.cumsum(order)[-1]) - total)
                    share = max(share, err / ((N + 8) * 2.0 ** -53 * total))
    print("largest share of the bound: %.3f" % share)
    assert share <= 1.0
