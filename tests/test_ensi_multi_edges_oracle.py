"""The reference side of the ensi_multi edge suite (tests/test_gpu_ensi_multi_edges.py), without a GPU: on the same named cases and
seeds the C oracle agrees with the independent numpy + LAPACK restatement (tools/make_ensi_multi_fixtures.ensi_multi) under the
project's measure, and every case meets the condition that keeps it from being vacuous."""
import numpy as np
import pytest

from tests import ensi_multi_cases as K
from tests import ensi_multi_golden as G

RESTATED = (["b_ebe", "b_ebesc", "c_ebe_65", "c_ebesc_65", "c_utem_65", "d_64", "d_65", "i_ebe", "i_utem"]
            + sorted(n for n in K.SPECS if n.startswith("h_")))


@pytest.mark.parametrize("name", RESTATED)
def test_oracle_agrees_with_the_restatement(name):
    pytest.importorskip("scipy")
    G.compare(K.reference(name), K.restatement(K.case(name)))
    K.assert_not_vacuous(name)


@pytest.mark.parametrize("name", sorted(n for n in K.SPECS if n not in RESTATED and n[0] != "k" and n != "f_ebe_4097"))
def test_case_is_not_vacuous(name):
    """the remaining cases of the GPU suite: their conditions hold on the oracle (f_utem_260: on its committed expected values)"""
    K.assert_not_vacuous(name)


def test_singular_cases_are_singular_for_the_oracle():
    from oracle import oracle as O
    for name in ("k_sing_lds", "k_sing_huge"):
        c = K.case(name)
        counts, _ = K.selection_counts(c)
        assert (counts == c["plat"].size).all() and (counts > 64).all() == (name == "k_sing_huge")
        with pytest.raises(O.OracleSingular):
            K.oracle(c)


def test_utem260_fixture_is_the_restatement():
    """the committed expected values of f_utem_260 (the oracle needs 11 s for this case) are what the restatement gives today"""
    pytest.importorskip("scipy")
    np.testing.assert_array_equal(K.reference("f_utem_260"), K.restatement(K.case("f_utem_260")))


def test_builder_follows_its_arguments():
    c = K.make_case("utem", 12, 3, 7, 1, 40000, 5, True, grid_shape=(3, 4))
    assert c["background"].shape == (12, 3) and c["pobs"].shape == (7,) and list(c["shape"]) == [3, 4, 3]
    assert list(c["params"]) == [40000, 0, 0, 5, 1.0] and int(c["ctype"]) == 0
    assert c["pratios"].min() >= 0.1 and c["pratios"].max() <= 1 and c["bratios"].min() >= 0.5 and c["bratios"].max() <= 1.5
    m = K.make_case("ebe", 12, 3, 7, 1, 40000, 5, False, ctype=1)
    assert m["pobs"].shape == (7, 3) and m["blat"].max() > 1000 and list(K.with_params(m, allow=True)["params"][3:]) == [5, 1.0]
