"""tests/oi_union_split_cases.py on the CPU: every construction reaches the (c, nE, extras per cell) it claims, the pivot cases are singular
for the oracle, the list case splits as its docstring says, and the Cressman case selects what the Barnes geometry was derived for."""
import numpy as np
import pytest

from tests import oi_union_split_cases as K
from tests.test_gpu_oi_union_solve import _oracle, _radius


@pytest.mark.parametrize("name", sorted(K.TILES))
def test_tile_construction(name):
    case = K.build(name)
    assert np.isfinite(_oracle(case, K.MP)[np.isfinite(case["bg"])]).all()


def test_one_cell_extremes_and_list_case():
    assert np.isfinite(K.one_cell()["bg"]).sum() == 1
    ext = K.extreme_cases()
    assert len(ext) == 28 and all(np.argmax(c["obs"] - c["pbg"]) == k for k, c in enumerate(ext))
    K.list_case()


def test_pivot_cases_are_singular():
    from oracle import oracle as O
    assert len(K.negative_cases()) == 19
    cases = K.pivot_cases()
    assert len(cases) == 19
    for c in cases:
        with pytest.raises(O.OracleSingular):
            _oracle(c, K.MP)


def test_cressman_reaches_what_barnes_reaches():
    from oracle import oracle as O
    h = K.cressman_h()
    assert O.Struct("Cressman", h).localization_distance() == np.float32(_radius())
    c = K.build("c19_e12")
    S = c["plat"].size
    og, op = O.Pts(c["lats"].ravel(), c["lons"].ravel()), O.Pts(c["plat"], c["plon"])
    ref, _ = O.oi_full_generic(og, c["bg"].ravel(), np.ones(64, np.float32), op, c["obs"], c["ratios"], c["pbg"], np.ones(S, np.float32),
                               O.Struct("Cressman", h), K.MP)
    assert np.isfinite(ref).all()
