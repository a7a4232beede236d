"""CPU-only: the cases of tests/test_gpu_structure_corr_many.py cannot pass vacuously.  With the oracle's corr
(orc_corr_generic) in place of the device, every case, first point and (NaN variant of it, flag) has at least a quarter of its
1000 values strictly inside (0, 1), an exact 0, and an exact 1 at the first point itself (tests/structure_corr_cases.py: vacuous)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import structure_corr_cases as K


@pytest.mark.parametrize("case", K.CASES, ids=repr)
def test_case_is_not_vacuous(case):
    for centre in case.centres:
        lats, lons, elevs, lafs = K.pool(centre)
        x, y, z = O.convert_coordinates(lats, lons, O.Geodetic)
        st = case.oracle(O, *centre)
        for variant, background in K.COMBOS:
            elev, laf = K.P1_VARIANTS[variant]
            p1 = (x[0], y[0], z[0], elev, laf)
            values = [st.corr(p1, (x[i], y[i], z[i], np.float32(elevs[i]), np.float32(lafs[i])), background) for i in range(K.N)]
            why = K.vacuous(values, True, case.cv and background)
            assert why is None, (case, centre, variant, background, why)
            if case.cv and background:   # the two flags differ on a point closer than the cross-validation distance
                plain = [st.corr(p1, (x[i], y[i], z[i], np.float32(elevs[i]), np.float32(lafs[i])), 0) for i in range(K.N)]
                assert any(a != b for a, b in zip(plain, values))


def test_spatial_first_points_lie_in_cells_of_different_scale():
    cells = [K._field_index(O, *c) for c in K.SPATIAL_CENTRES]
    assert len(set(cells)) == 3 and len({float(K.FIELD_H[c]) for c in cells}) == 3
    assert K.FIELD_H.min() < 0.75 * K.H and K.FIELD_H.max() > 1.25 * K.H   # +-30 %


def test_pool_holds_what_the_cases_need():
    lats, lons, elevs, lafs = K.pool(K.CENTRE)
    assert (lats[0], lons[0], elevs[0], lafs[0]) == (K.CENTRE[0], K.CENTRE[1], K.P1_ELEV, K.P1_LAF)   # one second point IS the first
    assert np.isnan(elevs).sum() > 50 and np.isnan(lafs).sum() > 50
    assert np.abs(lats - K.CENTRE[0]).max() > 4.4          # beyond the widest localization distance (Powerlaw, 392 km)
    assert max(K.SIZES) == K.N and max(y * x for y, x in K.GRIDS) <= K.N
