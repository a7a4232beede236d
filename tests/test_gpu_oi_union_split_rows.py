"""k_oi_union with every row of the shared factorisation split over two lanes (csrc/oi_union.h, GPP_UNION_SPLIT): the edges the split adds,
on single tiles built for them (tests/oi_union_split_cases.py says which, and which the 32-column form cannot be given), against

  * the CPU oracle, tolerance of tests/test_gpu_oi_union_solve.py (RTOL 1e-5 over a floor of 1e-3, NaN pattern equal), and
  * the bits the library had before the split, recorded once on the GPU by tools/make_oi_union_split_rows_golden.py into
    tests/golden/oi_union_split_rows_parent.npz: the split changes which lane holds an entry, not one operand or the order of its
    multiply-adds, so np.array_equal must hold."""
import functools
import os

import numpy as np
import pytest

from tests import oi_union_split_cases as K
from tests.test_gpu_oi_union_solve import H, _check, _oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oi_union_split_rows_parent.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    if not os.path.exists(GOLDEN):
        pytest.skip("tests/golden/oi_union_split_rows_parent.npz is missing: record it with tools/make_oi_union_split_rows_golden.py")
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def _same_bits(name, out):
    ref = _golden()[name]
    assert out.dtype == np.float32 and ref.dtype == np.float32 and out.shape == ref.shape
    assert np.array_equal(out, ref, equal_nan=True), "%s: %d values differ from the recorded bits" % (name, int((out != ref).sum()))


def _first_pass(s):
    assert s["union_kernel_ms"] > 0 and s["fallback_tiles"] == 0 and s["solves"] == 1, s      # one tile, one shared factorisation


def test_the_cases_cover_the_edges_of_the_split():
    assert set(K.CORE_ONLY) == {1, 3, 4, 5, 17, 18, 19, 28, 32}
    assert any(c < 18 and c + nE > 18 for c, _, _, (nE, _) in K.TILES.values())            # extras rows of a lower-half core in the upper half
    us = {c + nE for c, _, _, (nE, _) in K.TILES.values()}
    assert {33, 36, 39, 40} <= us                                                          # late columns: one, four, seven, eight; lane 61 idle / live
    late = [c for c, _, _, (nE, _) in K.TILES.values() if c + nE > 32]
    assert min(late) == 21 and max(late) == 31 and any(c % 2 for c in late) and any(c % 2 == 0 for c in late)


@pytest.mark.parametrize("name", sorted(K.TILES))
def test_tile(name):
    case = K.build(name)
    out, _, s = K.run(case)
    print(name, s)
    _first_pass(s)
    _check(out, _oracle(case, K.MP))
    out2, _, _ = K.run(case)
    assert np.array_equal(out, out2, equal_nan=True)
    _same_bits(name, out)


@pytest.mark.parametrize("name", K.WITH_VARIANCE)
def test_tile_with_variance(name):
    from oracle import oracle as O
    c = K.build(name)
    out, var, s = K.run(c, variance=True, seed=len(name))
    _first_pass(s)
    bvar = np.random.default_rng(len(name)).uniform(0.5, 2, c["bg"].shape).astype(np.float32)
    og, op = O.Pts(c["lats"].ravel(), c["lons"].ravel()), O.Pts(c["plat"], c["plon"])
    ref, rvar = O.oi_full(og, c["bg"].ravel(), bvar.ravel(), op, c["obs"], c["ratios"], c["pbg"], np.ones(c["plat"].size, np.float32), O.Barnes(H), K.MP)
    _check(out, ref.reshape(out.shape))
    _check(var, rvar.reshape(var.shape))
    _same_bits(name + "_full", out)
    _same_bits(name + "_var", var)


def test_one_updating_cell():
    case = K.one_cell()
    out, _, s = K.run(case)
    _first_pass(s)
    assert s["cells_updated"] == 1, s
    _check(out, _oracle(case, K.MP))
    _same_bits("one_cell", out)


def test_no_extrapolation_with_the_extreme_in_every_row():
    from oracle import oracle as O
    outs = []
    for c in K.extreme_cases():
        out, _, s = K.run(c, allow_extrapolation=False)
        _first_pass(s)
        og, op = O.Pts(c["lats"].ravel(), c["lons"].ravel()), O.Pts(c["plat"], c["plon"])
        _check(out, O.oi(og, c["bg"].ravel(), op, c["obs"], c["ratios"], c["pbg"], O.Barnes(H), K.MP, False).reshape(out.shape))
        outs.append(out)
    _same_bits("extreme", np.stack(outs))


def test_non_positive_pivot_in_either_half():
    """A negative diagonal entry in each of the nineteen rows in turn (row 18 is an upper lane's): the factorisation reports the pivot, the
    call is redone by k_oi's pivoted LU and returns what it returned before the split -- a Cholesky that went on would return NaNs.  Then
    the pairs of equal rows, built as test_non_positive_pivot builds its own (the oracle finds every one singular): each ends as it did
    before the split, raising `singular` or not (tests/oi_union_split_cases.py:pivot_cases); some raise.  The next call is clean."""
    from oracle import oracle as O
    ends = [K.ending(c) for c in K.negative_cases()]
    assert not any(e[0] for e in ends) and all(np.isfinite(e[1]).all() for e in ends)
    _same_bits("neg_out", np.stack([e[1] for e in ends]))
    cases = K.pivot_cases()
    for c in cases:
        with pytest.raises(O.OracleSingular):
            _oracle(c, K.MP)
    ends = [K.ending(c) for c in cases]
    _same_bits("dup_raised", np.array([e[0] for e in ends], np.float32))
    assert _golden()["dup_raised"].any()
    _same_bits("dup_out", np.stack([e[1] for e in ends]))
    ok = K.build("c19")
    out, _, s = K.run(ok)
    _first_pass(s)
    _same_bits("c19", out)


def test_list_passes_on_either_side_of_the_split():
    case = K.list_case()
    out, _, s = K.run(case)
    print(s)
    assert s["union_kernel_ms"] > 0 and s["fallback_tiles"] == 1 and s["fallback_subtiles"] == 0 and s["solves"] == K.LIST_SOLVES, s
    _check(out, _oracle(case, K.MP))
    _same_bits("list", out)


def test_cressman_with_extras():
    """the generic (non-PLAIN) instantiation: c = 19, twelve extras"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = K.build("c19_e12")
    h = K.cressman_h()
    out, _, s = K.run(c, structure=gridpp.CressmanStructure(h))
    _first_pass(s)
    S = c["plat"].size
    og, op = O.Pts(c["lats"].ravel(), c["lons"].ravel()), O.Pts(c["plat"], c["plon"])
    ref, _ = O.oi_full_generic(og, c["bg"].ravel(), np.ones(64, np.float32), op, c["obs"], c["ratios"], c["pbg"], np.ones(S, np.float32),
                               O.Struct("Cressman", h), K.MP)
    _check(out, np.asarray(ref).reshape(out.shape))
    _same_bits("cressman_c19_e12", out)
