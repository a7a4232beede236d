"""CPU checks that go with tests/test_gpu_oi_pair_table.py: the geometry the GPU assertions rely on, from the oracle's selections and the
restated index (tests/oi_pair_table_cases.py: geometry)."""
import pytest

from tests import oi_pair_table_cases as T


@pytest.mark.parametrize("name", T.NAMES)
def test_default_window_holds_every_pair(name):
    asked, used, per_cell, whole, fullest, corner, least = T.geometry(name)
    print(name, "window asked %d, in use %d; bins between two observations of one cell %d, of the grid %d; fullest bin %d; corner bin %s"
          % (asked, used, per_cell, whole, fullest, corner))
    assert used >= 1 and whole <= used          # no pair of any union lies outside the window: pair_fallback_items == 0


@pytest.mark.parametrize("name", T.WINDOW1_MISSES)
def test_window_one_must_miss(name):
    assert T.geometry(name)[6] >= 2             # every cell selects two observations two bins apart: every work item misses


def test_the_cases_cover_the_list():
    mps = {T.mp_of(n) for n in T.NAMES}
    assert {8, 30, 32, 40, 50} <= mps
    assert {T.build(n)["bg"].shape for n in T.NAMES} >= {(8, 8), (16, 16)}
    sizes = {T.build(n)["plat"].size for n in T.NAMES}
    assert {1, 2} <= sizes and any(35 <= s <= 62 for s in sizes)
    assert any(T.build(n)["plat"].size < T.mp_of(n) for n in T.NAMES)
    # observations in a corner bin of the index (a window clamped on two sides) take part in a union
    assert sum(T.geometry(n)[5] for n in T.NAMES) >= 5
    # all observations in one bin (S = 1 and S = 3), and a bin that holds most of a larger set
    assert T.geometry("u1")[4] == 1 and T.geometry("three_one_bin")[4] == 3 and T.geometry("one_bin")[4] >= 25
    c = T.build("ties2_first_pass")
    assert len({(a, b) for a, b in zip(c["plat"], c["plon"])}) < c["plat"].size          # two observations at one place
    import numpy as np
    assert np.isnan(T.build("nan_elevation")["pelevs"]).any() and T.build("nan_elevation")["st"][1] == 200.0
    assert T.build("laf_factor")["st"][2] == 0.5 and np.isnan(T.build("laf_factor")["plafs"]).any()
