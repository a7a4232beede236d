"""The OI gain on the device (gridpp_amd/csrc/oi_gain.hip) at its pivot, tile-shape, field-count and size edges: the cases of
tests/oi_gain_cases.py (tests/test_oi_gain_cases_oracle.py shows on the CPU that they reach what they claim).

A. Pivots that leave the diagonal (chain, chain-permuted, cressman-chain), every cell:
   counts() / indices() equal the oracle's selection; weights() equal numpy.linalg.solve((P + R)^T, g) in double within 1e-9 max|w| per
   cell.  Where that number comes from: tests/test_gpu_staticcorr_parity.py pins the device's Barnes and Cressman correlations bit-equal
   to the oracle's, and the one-station cells below pin it again for g (w = rho / (1 + r) within 2 ulp of double only if the device's
   rho IS the oracle's float32).  The two solves then start from identical matrices and differ by the order of elimination, of order
   n^2 cond 2^-53 = 3e-12 at n = 12 and cond = 200 (asserted <= 200 on the CPU); one float32 intermediate would show as 6e-8.  1e-9 is
   300 times the first and 60 times below the second.  Every test prints its largest error over the bound.
   analysis_variance(ones) = 1 - w . g within one float32 ulp plus n 1e-9 max|w|; apply for 1 and 17 fields against apply_reference and,
   one field, against the oracle under the project's measure.
B. A 13 x 70 grid under GPP_TILE_WSHIFT = 0 ... 6 and without: the same selections, weights within the bound of A, every analysis the
   oracle's; grids of one row and of one column.
C. max_points 62 with selection sizes in every residue mod 8: apply at 15 ... 129 fields against apply_reference -- plain numpy in
   double from the gain's OWN indices() and weights() -- within spacing(|inc|) + spacing(|want|) per element (the two double sums
   differ in their order of summation only, so the float32 increments are equal or adjacent, and the float32 add moves the result by at
   most one more ulp); cells without a selection and invalid background values bit for bit; no element is left out.
D. Points backgrounds of 1, 63, 64, 65 points; max_points 32."""
import functools

import numpy as np
import pytest

from tests import oi_gain_cases as K
from tests.test_gpu_oi_parity import check

pytestmark = pytest.mark.gpu
F = np.float32
ULP = 2.0 ** -52
PIVOT_CASES = {"chain": lambda: K.chain(), "chain-permuted": lambda: K.chain(True), "cressman-chain": K.cressman_chain}


def build(case):
    import gridpp_amd as gridpp
    bgrid, points, st = case.device(gridpp)
    return gridpp.optimal_interpolation_gain(bgrid, points, case.ratios, st, case.max_points)


@functools.lru_cache(maxsize=None)
def built(case):
    """the gain of a case by the default dispatch (never called under a path override), with its planes read back once"""
    gain = build(case)
    counts, indices, weights = gain.counts(), gain.indices(), gain.weights()
    assert counts.dtype == np.int32 and indices.dtype == np.int32 and weights.dtype == np.float64
    assert counts.shape == case.shape and indices.shape == weights.shape == case.shape + (case.max_points,)
    for a in (counts, indices, weights):
        a.setflags(write=False)
    return gain, counts, indices, weights


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    view = np.uint32 if a.dtype.itemsize == 4 else np.uint64
    np.testing.assert_array_equal(a.view(view), b.view(view))


def oracle_indices(case):
    idx = np.full((case.cells, case.max_points), -1, np.int32)
    for cell, sel in enumerate(case.selections[0]):
        idx[cell, :len(sel)] = sel
    return idx.reshape(case.shape + (case.max_points,))


def check_selection(case, counts, indices):
    """counts and index lists (ascending, -1 behind the selection) are the oracle's at every cell"""
    assert not case.selections[1].any()
    np.testing.assert_array_equal(counts, case.counts)
    np.testing.assert_array_equal(indices, oracle_indices(case))


def check_apply(got, counts, indices, weights, bg, pobs, pbg, allow):
    """every element against apply_reference; what an analysis does not touch, bit for bit"""
    want, tol, changed = K.apply_reference(counts, indices, weights, bg, pobs, pbg, allow)
    assert got.shape == want.shape and got.dtype == np.float32
    same_bits(got[~changed], np.asarray(bg)[~changed])
    err = np.abs(got[changed].astype(np.float64) - want[changed].astype(np.float64))
    print("apply: %d elements, %d passed through, max err / tol = %.3f" % (got.size, (~changed).sum(), np.max(err / tol[changed], initial=0)))
    assert np.isfinite(got[changed]).all() and (err <= tol[changed]).all()
    assert changed.sum() + (~changed).sum() == got.size


# ---- A. pivots that leave the diagonal -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PIVOT_CASES)
def test_pivot_case_selection_and_weights(name):
    case = PIVOT_CASES[name]()
    gain, counts, indices, weights = built(case)
    check_selection(case, counts, indices)
    assert gain.largest_selection == counts.max() == case.S
    n, w = counts.ravel(), weights.reshape(case.cells, -1)
    wref, _ = case.reference_weights
    assert (w[np.arange(case.max_points)[None, :] >= n[:, None]] == 0).all()          # 0 behind the selection
    # one station: the device's g is the oracle's float32 rho, the premise of the bound below
    ones = np.flatnonzero(n == 1)
    assert ones.size >= 10
    for cell in ones:
        (s,) = case.selections[0][cell]
        want = case.rho(cell, (s,))[0] / (1.0 + float(case.ratios[s]))
        assert abs(w[cell, 0] - want) <= 2 * ULP * abs(want), (cell, w[cell, 0], want)
    # every cell, grouped by distinct selection (the reference solves once per group)
    worst = 0.0
    for sel, cells in case.groups.items():
        k = len(sel)
        err = np.abs(w[cells, :k] - wref[cells, :k]).max(axis=1)
        bound = K.WEIGHT_RTOL * np.abs(wref[cells, :k]).max(axis=1)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (sel, case.pivots[sel][0], float((err / bound).max()))
    print("%s: %d cells in %d groups, max |dw| / (1e-9 max|w|) = %.3g" % (name, sum(map(len, case.groups.values())), len(case.groups), worst))


@pytest.mark.parametrize("name", PIVOT_CASES)
def test_pivot_case_variance(name):
    case = PIVOT_CASES[name]()
    gain, counts, _, _ = built(case)
    wref, aref = case.reference_weights
    got = gain.analysis_variance(np.ones(case.shape, F))
    assert got.dtype == np.float32 and got.shape == case.shape
    n = counts.ravel()
    want = np.where(n > 0, 1.0 - aref, 1.0)
    tol = np.spacing(np.abs(want).astype(F)).astype(np.float64) + n * K.WEIGHT_RTOL * np.abs(wref).max(axis=1)
    err = np.abs(got.ravel().astype(np.float64) - want)
    print("%s: variance max err / tol = %.3f" % (name, (err / tol).max()))
    assert (err <= tol).all()
    assert (got.ravel()[n == 0] == 1).all() and (got.ravel()[aref > 1e-3] < 1).all() and (aref > 1e-3).sum() >= 300


@pytest.mark.parametrize("allow", [True, False], ids=["extrapolate", "clamp"])
@pytest.mark.parametrize("E", [1, 17])
@pytest.mark.parametrize("name", PIVOT_CASES)
def test_pivot_case_apply(name, E, allow):
    case = PIVOT_CASES[name]()
    gain, counts, indices, weights = built(case)
    bg, pobs, pbg = case.fields(E)
    if E == 1:
        got = gain.apply(bg[..., 0], pobs[:, 0], pbg[:, 0], allow)
        assert got.shape == case.shape
        check(got, case.oracle_analysis(bg[..., 0], pobs[:, 0], pbg[:, 0], allow))       # the oracle's analysis, the project's measure
        got = got[..., None]
    else:
        got = gain.apply(bg, pobs, pbg, allow)
    check_apply(got, counts, indices, weights, bg, pobs, pbg, allow)
    if not allow:
        assert (got != (gain.apply(bg, pobs, pbg, True) if E > 1 else gain.apply(bg[..., 0], pobs[:, 0], pbg[:, 0], True)[..., None])).any()


# ---- B. tile shapes ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tile_references():
    """the oracle's analyses of the tile-shape case: one field, seventeen fields, the variance"""
    case = K.tile_shapes()
    bg1, pobs1, pbg1 = case.fields(1)
    bg17, pobs17, pbg17 = case.fields(17)
    one, var = case.oracle_analysis(bg1[..., 0], pobs1[:, 0], pbg1[:, 0], variance=True)
    stack = [case.oracle_analysis(bg17[..., e], pobs17[:, e], pbg17[:, e]) for e in range(17)]
    return one, var, stack


@pytest.mark.parametrize("wshift", (None,) + K.TILE_SHIFTS, ids=lambda w: "default" if w is None else "w%d" % w)
def test_tile_shapes(wshift, monkeypatch):
    import gridpp_amd as gridpp
    case = K.tile_shapes()
    _, counts0, indices0, weights0 = built(case)          # (built before the override is set)
    if wshift is None:
        gain, counts, indices, weights = built(case)
    else:
        monkeypatch.setenv("GPP_TILE_WSHIFT", str(wshift))
        gain = build(case)
        assert "GPP_TILE_WSHIFT" in gridpp.active_overrides()
        counts, indices, weights = gain.counts(), gain.indices(), gain.weights()
    check_selection(case, counts, indices)
    np.testing.assert_array_equal(counts, counts0)
    np.testing.assert_array_equal(indices, indices0)
    bound = K.WEIGHT_RTOL * np.abs(weights0).max(axis=-1)
    err = np.abs(weights - weights0).max(axis=-1)
    identical = np.array_equal(weights.view(np.uint64), weights0.view(np.uint64))
    print("wshift %s: weights %s the unforced gain's, max |dw| / (1e-9 max|w|) = %.3g" %
          (wshift, "bit-identical to" if identical else "differ from", (err / bound).max()))
    assert (err <= bound).all()
    assert gain.largest_selection == counts.max() == K.TILE_MAX_POINTS
    one, var, stack = tile_references()
    bg1, pobs1, pbg1 = case.fields(1)
    bg17, pobs17, pbg17 = case.fields(17)
    check(gain.apply(bg1[..., 0], pobs1[:, 0], pbg1[:, 0]), one)
    check(gain.analysis_variance(np.ones(case.shape, F)), var)
    out = gain.apply(bg17, pobs17, pbg17)
    for e in range(17):
        check(np.ascontiguousarray(out[..., e]), stack[e])
    check_apply(out, counts, indices, weights, bg17, pobs17, pbg17, True)


@pytest.mark.parametrize("shape", K.LINE_GRIDS, ids=lambda s: "%dx%d" % s)
def test_grids_of_one_row_or_column(shape):
    case = K.line_grid(shape)
    gain, counts, indices, weights = built(case)
    check_selection(case, counts, indices)
    assert gain.largest_selection == counts.max()
    for E in (1, 17):
        bg, pobs, pbg = case.fields(E)
        out = gain.apply(bg, pobs, pbg) if E > 1 else gain.apply(bg[..., 0], pobs[:, 0], pbg[:, 0])[..., None]
        for e in range(E):
            check(np.ascontiguousarray(out[..., e]), case.oracle_analysis(bg[..., e], pobs[:, e], pbg[:, e]))
    bg, pobs, pbg = case.fields(1)
    check(gain.analysis_variance(np.ones(case.shape, F)), case.oracle_analysis(bg[..., 0], pobs[:, 0], pbg[:, 0], variance=True)[1])


# ---- C. field counts and selection sizes of the two apply kernels ------------------------------------------------------------------------
def test_wide_case_selection_sizes():
    case = K.wide()
    gain, counts, indices, _ = built(case)
    check_selection(case, counts, indices)
    assert {int(n) % 8 for n in counts.ravel() if n > 0} == set(range(8))
    assert counts.max() == 62 == gain.largest_selection and (counts == 0).any()


@pytest.mark.parametrize("allow", [True, False], ids=["extrapolate", "clamp"])
@pytest.mark.parametrize("E", K.WIDE_FIELDS)
def test_wide_field_counts(E, allow):
    case = K.wide()
    gain, counts, indices, weights = built(case)
    bg, pobs, pbg = K.wide_background(E)
    got = gain.apply(bg, pobs, pbg, allow)
    check_apply(got, counts, indices, weights, bg, pobs, pbg, allow)
    bad = ~np.isfinite(bg)
    assert bad.sum() >= 4 and bad[..., E - 1].any() and (E <= 64 or bad[..., 64].any())
    same_bits(got[bad], bg[bad])
    same_bits(got[counts == 0], bg[counts == 0])
    if not allow:     # the clamp was at work: in the first field, in the last one and in the first of the second pass of the lanes
        free = K.apply_reference(counts, indices, weights, bg, pobs, pbg, True)[0]
        bound = (free != got) & ~bad
        print("clamped: %d of %d elements" % (bound.sum(), bound.size))
        assert bound.sum() >= 2 * E and all(bound[..., e].any() for e in {0, E - 1, min(64, E - 1)})
    if E == 65:      # once more from device tensors: the same bits
        import torch
        dev = gain.apply(*[torch.from_numpy(np.array(a)).cuda() for a in (bg, pobs, pbg)], allow)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float32
        same_bits(dev.cpu().numpy(), got)


# ---- D. sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.POINT_COUNTS)
def test_points_background_sizes(n):
    case = K.points_background(n)
    gain, counts, indices, weights = built(case)
    assert counts.shape == (n,) and indices.shape == (n, case.max_points) == weights.shape
    check_selection(case, counts, indices)
    assert gain.largest_selection == counts.max()
    for E in (1, 17):
        bg, pobs, pbg = case.fields(E)
        out = gain.apply(bg, pobs, pbg) if E > 1 else gain.apply(bg[..., 0], pobs[:, 0], pbg[:, 0])[..., None]
        assert out.shape == (n, E)
        for e in range(E):
            check(np.ascontiguousarray(out[..., e]), case.oracle_analysis(bg[..., e], pobs[:, e], pbg[:, e]))
        check_apply(out, counts, indices, weights, bg, pobs, pbg, True)


def test_max_points_32():
    case = K.max_points_32()
    assert case.counts.max() == 32                     # (from the oracle)
    gain, counts, indices, weights = built(case)
    check_selection(case, counts, indices)
    assert gain.largest_selection == counts.max() == 32 == gain.max_points
    for E in (1, 16):
        bg, pobs, pbg = case.fields(E)
        out = gain.apply(bg, pobs, pbg) if E > 1 else gain.apply(bg[..., 0], pobs[:, 0], pbg[:, 0])[..., None]
        for e in range(E):
            check(np.ascontiguousarray(out[..., e]), case.oracle_analysis(bg[..., e], pobs[:, e], pbg[:, e]))
        check_apply(out, counts, indices, weights, bg, pobs, pbg, True)
