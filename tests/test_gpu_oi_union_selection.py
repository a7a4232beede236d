"""The selection machinery of k_oi_union's scan -- worst_slot (minima without NaN handling), the eviction path of run_chunk, end_bulk -- and
the triangle-index table of its P build (csrc/oi_union.h, oi_small.h), on the single tiles and the 16 x 16 grid of
tests/oi_union_selection_cases.py (tests/test_oi_union_selection_cases_oracle.py checks on the CPU what each case claims).  Every case is
compared

  * with the CPU oracle: RTOL 1e-5 over a floor of 1e-3, NaN pattern equal (the comparison of the parity tests);
  * bit for bit with its run under GPP_OI_NO_BULK_CERT, the other form of the bulk loop;
  * bit for bit with tests/golden/oi_union_selection_parent.npz, recorded once with the library of the commit before these changes by
    tools/make_oi_union_selection_golden.py: none of them may change a selection or an operand."""
import functools
import os

import numpy as np
import pytest

from tests import oi_union_selection_cases as K
from tests.test_gpu_oi_union_bulk_cert import _check

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oi_union_selection_parent.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def _same_bits(name, out):
    ref = _golden()[name]
    assert out.dtype == np.float32 and ref.dtype == np.float32 and out.shape == ref.shape
    assert np.array_equal(out, ref, equal_nan=True), "%s: %d values differ from the recorded bits" % (name, int((out != ref).sum()))


def test_golden_file_holds_every_case():
    assert set(_golden()) == set(K.CASES) | {"cressman_" + K.CRESSMAN}


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_case(name):
    out, out0, s = K.run(name)
    print(name, s)
    # (a tile kernel ran.  max_points 40 and 50 -- form48, form64 -- cannot run on the 32-column form, which holds 32 columns: with them
    #  this says that the 48- / 64-column instantiation ran; the statistics name no instantiation)
    assert s["union_kernel_ms"] > 0, s
    if K.mp_of(name) <= 32:
        # more than 40 observations in the selections of one tile: no shared factorisation of the 32-column form holds them
        if K.facts(name)[3] > K.DECLINED_UNION and K.build(name)["bg"].shape == (8, 8):
            assert s["solves"] > 1, s
    _check(out, K.oracle(name))
    assert np.array_equal(out, out0, equal_nan=True)
    _same_bits(name, out)


def test_cressman_generic_p_build():
    """the generic (non-PLAIN) instantiation: its scan evicts too, its P build reads the table"""
    from oracle import oracle as O
    st, ost = K.cressman()
    c = K.build(K.CRESSMAN)
    out, out0, s = K.run(K.CRESSMAN, st)
    assert s["union_kernel_ms"] > 0, s
    S = c["plat"].size
    og, op = O.Pts(c["lats"].ravel(), c["lons"].ravel()), O.Pts(c["plat"], c["plon"])
    ref, _ = O.oi_full_generic(og, c["bg"].ravel(), np.ones(64, np.float32), op, c["obs"], c["ratios"], c["pbg"], np.ones(S, np.float32), ost, K.mp_of(K.CRESSMAN))
    _check(out, np.asarray(ref).reshape(out.shape))
    assert np.array_equal(out, out0, equal_nan=True)
    _same_bits("cressman_" + K.CRESSMAN, out)
