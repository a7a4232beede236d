"""The cases of tests/oi_gain_cases.py reach what they claim (no GPU): from the oracle alone, the pivot orders of the chains leave the
diagonal by a safe margin on well-conditioned matrices and no selection sits on a tie; the selection sizes of the wide case hold every
residue mod 8 and 62; the sizes of the last group are what they are named after.  The plain references are checked against closed forms
and against the oracle's own analysis."""
import numpy as np
import pytest

from tests import oi_gain_cases as K

F = np.float32
PIVOT_CASES = {"chain": lambda: K.chain(), "chain-permuted": lambda: K.chain(True), "cressman-chain": K.cressman_chain}


# ---- the restated pivot rule -----------------------------------------------------------------------------------------------------------
def test_gj_pivot_order_on_matrices_done_by_hand():
    assert K.gj_pivot_order([[2.0]]) == ([0], [1.0])
    # column 0: |3| beats |1|, row 1 is the pivot (margin 2 / 3); row 0 becomes (0, 2 - 4 / 3) and takes step 1
    order, margins = K.gj_pivot_order([[1.0, 2.0], [3.0, 4.0]])
    assert order == [1, 0] and margins == pytest.approx([2 / 3, 1.0])
    # equal entries: the lowest row
    order, margins = K.gj_pivot_order([[1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [-1.0, 0.0, 1.0]])
    assert order == [0, 1, 2] and margins[0] == 0.0
    # a used row never comes back, whatever it holds: after step 0 row 0 still has the largest entry of column 1
    order, _ = K.gj_pivot_order([[4.0, 9.0], [1.0, 3.0]])
    assert order == [0, 1]
    # the elimination is the kernel's: with the recorded order, E A = the permutation with its ones at (p_k, k)
    rng = np.random.default_rng(0)
    A = rng.normal(0, 1, (7, 7))
    order, margins = K.gj_pivot_order(A)
    assert sorted(order) == list(range(7)) and order != list(range(7)) and min(margins) > 0
    lu_order = []                         # Gaussian elimination with partial pivoting takes the same rows
    M, free = A.copy(), list(range(7))
    for k in range(7):
        p = max(free, key=lambda r: abs(M[r, k]))
        free.remove(p)
        lu_order.append(p)
        for r in free:
            M[r] -= M[r, k] / M[p, k] * M[p]
    assert order == lu_order


# ---- A. pivots that leave the diagonal -----------------------------------------------------------------------------------------------
def test_the_chains_are_one_line_in_two_orders():
    a, b = K.chain(), K.chain(True)
    assert sorted(K.CHAIN_PERMUTATION) == list(range(K.CHAIN_STATIONS)) and list(K.CHAIN_PERMUTATION) != sorted(K.CHAIN_PERMUTATION)
    idx = np.array(K.CHAIN_PERMUTATION)
    np.testing.assert_array_equal(b.plon[idx], a.plon)
    np.testing.assert_array_equal(b.ratios[idx], a.ratios)
    assert (np.diff(a.plon) == K.CHAIN_SPACING).all() and not (np.diff(b.plon) > 0).all()
    np.testing.assert_array_equal(a.counts, b.counts)                       # the same cells see the same stations ...
    for sa, sb in zip(a.selections[0], b.selections[0]):                    # ... under other indices
        assert sorted(idx[list(sa)]) == list(sb)
    assert a.shape == K.CHAIN_GRID and a.oracle_structure.localization_distance() == pytest.approx(36456.5, abs=1.0)


@pytest.mark.parametrize("name", PIVOT_CASES)
def test_pivot_cases_leave_the_diagonal_by_a_safe_margin(name):
    case = PIVOT_CASES[name]()
    sels, ties = case.selections
    assert not ties.any()                                                   # (and max_points = every station: nothing is ever cut)
    assert case.max_points == case.S == K.CHAIN_STATIONS
    assert (case.counts == 0).sum() >= 100 and (case.counts == case.S).sum() >= 8 and (case.counts == 1).any()
    piv = case.pivots
    assert set(piv) == set(case.groups) and len(piv) >= 30
    identity = lambda sel: list(range(len(sel)))
    off = {sel for sel, (order, _, _) in piv.items() if order != identity(sel)}
    with_selection = sum(len(c) for c in case.groups.values())
    share = sum(len(case.groups[sel]) for sel in off) / with_selection
    orders = {tuple(piv[sel][0]) for sel in off}
    worst = min((m for sel in off for k, (p, m) in enumerate(zip(*piv[sel][:2])) if p != k), default=1.0)
    every = min(min(m) for _, m, _ in piv.values())
    cond = max(c for _, _, c in piv.values())
    print("%s: %d distinct selections, %.1f %% of %d cells off the diagonal, %d distinct orders, margins >= %.4f off / %.4f on the diagonal, "
          "cond <= %.1f" % (name, len(piv), 100 * share, with_selection, len(orders), worst, every, cond))
    assert share >= K.MIN_OFF_DIAGONAL_SHARE
    assert len(orders) >= 3
    assert worst >= K.MIN_MARGIN
    assert every >= 1e-3                                                    # no step at all is decided by a last bit
    assert cond <= K.MAX_COND
    full = tuple(range(case.S))
    assert full in piv and piv[full][0] != identity(full)
    # the three places of the kernel differ from the identity: some row is not in its own step (M[j][mystep]), some step not on its own
    # row (pj), and at a cell of such a selection g differs between the two (rho[pj] against rho[j])
    order = piv[full][0]
    cell = case.groups[full][0]
    g = case.rho(cell, full)
    assert any(order.index(r) != r for r in range(case.S)) and any(g[order[j]] != g[j] for j in range(case.S))


def test_pivot_orders_of_the_whole_line():
    """what a cell that selects all twelve stations does, for DESIGN.md 4.15"""
    full = tuple(range(K.CHAIN_STATIONS))
    assert K.chain().pivots[full][0] == [0, 1, 3, 2, 4, 5, 6, 7, 9, 8, 10, 11]
    assert K.chain(True).pivots[full][0] == [0, 1, 11, 3, 4, 5, 7, 6, 8, 9, 10, 2]
    assert K.cressman_chain().pivots[full][0] == K.CRESSMAN_FULL_ORDER


def test_cressman_chain_is_not_symmetric():
    case = K.cressman_chain()
    P = case.station_corr
    assert np.abs(P - P.T).max() > 0.05 and (P < 0).any() and (np.diag(P) == 1).all()
    asym = [sel for sel in case.groups if np.abs(case.matrix(sel) - case.matrix(sel).T).max() > 0.05]
    assert sum(len(case.groups[sel]) for sel in asym) >= 50                 # cells whose own matrix is not symmetric
    # the restated selection is the reference's: the oracle's analysis moves exactly the cells with a selection
    bg, pobs, pbg = case.fields(1)
    out = case.oracle_analysis(bg[..., 0], pobs[:, 0], pbg[:, 0])
    np.testing.assert_array_equal(out != bg[..., 0], case.counts > 0)


@pytest.mark.parametrize("name", PIVOT_CASES)
def test_reference_weights_reproduce_the_oracle(name):
    """w . d from the reference weights is the oracle's increment, and 1 - w . g its variance: the references of the GPU file are the
    operation the oracle performs (to the oracle's own float32 result)"""
    case = PIVOT_CASES[name]()
    w, a = case.reference_weights
    bg, pobs, pbg = case.fields(1)
    bg, pobs, pbg = bg[..., 0], pobs[:, 0], pbg[:, 0]
    out, var = case.oracle_analysis(bg, pobs, pbg, variance=True)
    idx = np.full((case.cells, case.max_points), -1, np.int32)
    for cell, sel in enumerate(case.selections[0]):
        idx[cell, :len(sel)] = sel
    want, tol, changed = K.apply_reference(case.counts, idx, w, bg[..., None], pobs[:, None], pbg[:, None], True)
    np.testing.assert_array_equal(changed[..., 0], case.counts > 0)
    assert (np.abs(out.astype(np.float64) - want[..., 0]) <= tol[..., 0]).all()
    vref = np.where(case.counts.ravel() > 0, 1.0 - a, 1.0)
    assert (np.abs(var.ravel() - vref) <= np.spacing(vref.astype(F))).all()
    # a cell with one station: w = rho / (1 + r) exactly as the closed form
    ones = np.flatnonzero(case.counts.ravel() == 1)
    assert ones.size
    for cell in ones:
        (s,) = case.selections[0][cell]
        assert w[cell, 0] == pytest.approx(case.rho(cell, (s,))[0] / (1.0 + float(case.ratios[s])), rel=1e-15)


# ---- the reference of an apply ---------------------------------------------------------------------------------------------------------
def test_apply_reference_by_hand():
    counts = np.array([2, 0, 1, 2], np.int32)
    indices = np.array([[0, 2], [-1, -1], [1, -1], [0, 1]], np.int32)
    weights = np.array([[0.5, 0.25], [0, 0], [2.0, 0], [0.5, 0.5]])
    pobs, pbg = np.array([[1.0], [3.0], [-1.0]], F), np.array([[0.0], [1.0], [1.0]], F)      # d = 1, 2, -2
    bg = np.array([[10.0], [20.0], [30.0], [np.nan]], F)
    want, tol, changed = K.apply_reference(counts, indices, weights, bg, pobs, pbg, True)
    assert list(changed[:, 0]) == [True, False, True, False]
    np.testing.assert_array_equal(want[:3, 0], np.array([10.0 + 0.5 - 0.5, 20.0, 30.0 + 4.0], F))
    assert np.isnan(want[3, 0]) and tol[0, 0] == np.spacing(F(0)) + np.spacing(F(10)) and tol[2, 0] == np.spacing(F(4)) + np.spacing(F(34))
    # the clamp of oi.cpp:318-334: cell 2 has the single innovation 2 and the increment 4 -> 2
    clamped, _, _ = K.apply_reference(counts, indices, weights, bg, pobs, pbg, False)
    np.testing.assert_array_equal(clamped[:3, 0], np.array([10.0, 20.0, 32.0], F))
    # maxInc < 0 and increment > 0 -> maxInc; minInc > 0 and increment < 0 -> minInc
    neg, _, _ = K.apply_reference(np.array([1], np.int32), np.array([[2]], np.int32), np.array([[-1.0]]), bg[:1], pobs, pbg, False)
    assert neg[0, 0] == F(10.0 - 2.0)
    low, _, _ = K.apply_reference(np.array([1], np.int32), np.array([[2]], np.int32), np.array([[2.0]]), bg[:1], pobs, pbg, False)
    assert low[0, 0] == F(10.0 - 2.0)                                       # minInc < 0 and increment -4 < minInc -> minInc
    pos, _, _ = K.apply_reference(np.array([1], np.int32), np.array([[0]], np.int32), np.array([[-1.0]]), bg[:1], pobs, pbg, False)
    assert pos[0, 0] == F(10.0 + 1.0)


# ---- B. tile shapes ------------------------------------------------------------------------------------------------------------------
def test_tile_shape_grid_cuts_every_tile_shape():
    case = K.tile_shapes()
    Y, X = case.shape
    assert (Y, X) == (13, 70) and case.S == K.TILE_STATIONS and case.max_points == K.TILE_MAX_POINTS
    assert all(Y % (64 >> w) != 0 for w in K.TILE_SHIFTS if (64 >> w) > 1)      # a partial last tile row at every height but 1
    assert X % 64 == 6 and X > 64                                           # a second, partial tile of the widest shape
    assert not case.selections[1].any()                                    # no cell on a tie: indices() is the oracle's set too
    assert case.counts.max() == K.TILE_MAX_POINTS and len(set(case.counts.ravel())) >= 4
    for shape in K.LINE_GRIDS:
        line = K.line_grid(shape)
        assert line.shape == shape and min(shape) == 1 and line.counts.max() > 1 and not line.selections[1].any()
    assert {s[1] >= 64 for s in K.LINE_GRIDS if s[0] == 1} == {True, False}      # both answers of the ny < 2 branch, and the nx < 2 one
    assert (70, 1) in K.LINE_GRIDS


# ---- C. field counts and selection sizes ---------------------------------------------------------------------------------------------
def test_wide_case_selection_sizes():
    case = K.wide()
    counts = case.counts
    assert case.max_points == K.WIDE_MAX_POINTS == 62 and counts.max() == 62 and (counts == 0).sum() >= 64
    assert not case.selections[1].any()
    assert {int(n) % 8 for n in counts.ravel() if n > 0} == set(range(8))
    assert {15, 16, 63, 64, 65, 128, 129} == set(K.WIDE_FIELDS)
    for E in K.WIDE_FIELDS:
        bg, pobs, pbg = K.wide_background(E)
        bad = np.argwhere(~np.isfinite(bg))
        assert set(bad[:, 2]) == {E - 1, 64} & set(range(E))
        with_sel = counts[bad[:, 0], bad[:, 1]] > 0
        assert with_sel.any() and not with_sel.all() and np.isnan(bg[~np.isfinite(bg)]).any() and np.isinf(bg[~np.isfinite(bg)]).any()
        assert np.isfinite(pobs).all() and np.isfinite(pbg).all() and pobs.shape == pbg.shape == (case.S, E)


# ---- D. sizes ------------------------------------------------------------------------------------------------------------------------
def test_sizes():
    assert K.POINT_COUNTS == (1, 63, 64, 65)
    for n in K.POINT_COUNTS:
        case = K.points_background(n)
        assert case.shape == (n,) and case.counts.max() >= 1 and not case.selections[1].any()
    case = K.max_points_32()
    assert case.max_points == 32 and case.counts.max() == 32 and (case.counts < 32).any() and not case.selections[1].any()
