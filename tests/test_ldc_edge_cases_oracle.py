"""The fixtures of tests/ldc_edge_cases.py reach what they claim (no GPU): the restatement of tests/ldc_ref.py shows the pair counts of
the ladder and the branches each quantile pair takes there, the rho totals of 0 in the zero-rho cells, the branch of every threshold
cell as derived by hand, and the oracle's neighbour lists at exactly the localization distance."""
import numpy as np
import pytest

from tests import ldc_edge_cases as K
from tests import ldc_ref as R

F = np.float32


# ---- 1. the ladder --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounded", [False, True], ids=["tiefree", "rounded"])
def test_ladder_counts_and_branches(rounded):
    fx = K.ladder(rounded)
    assert fx.bg.shape == (10, 30) and fx.bg.size > 256                      # a second workgroup of 256 cells
    assert fx.px.size == sum(K.LADDER_COUNTS)
    for q, reached in K.LADDER_QUANTILES.items():
        out, tags, counts, sums = fx.restate(*q)
        np.testing.assert_array_equal(counts.reshape(fx.bg.shape), np.broadcast_to(K.LADDER_COUNTS, fx.bg.shape))
        assert set(tags) == reached[rounded], (q, set(tags))
        four = (tags == R.B4).reshape(fx.bg.shape)
        if q == (0.0, 1.0):
            # every count from 2 up has a branch-4 cell (tie-free count 1 too; rounded, its one fcst value is 0 and nothing lies below it)
            without = [n for k, n in enumerate(K.LADDER_COUNTS) if not four[:, k].any()]
            assert without == ([1] if rounded else []), without
            assert all(four[:, k].sum() >= 2 for k, n in enumerate(K.LADDER_COUNTS) if n >= 3)
        if q == (0.5, 0.5):
            assert (sums["sum_r"] == 0).all() and not four.any()             # d0 == d1: the lone (0, 0) point everywhere
        assert np.isfinite(out).all()


def test_ladder_sits_on_the_edges_of_the_kernels():
    c = set(K.LADDER_COUNTS)
    assert {K.LDS_MAX - 1, K.LDS_MAX, K.LDS_MAX + 1} <= c                     # the hand-over between the two finishing kernels
    assert {1, 2, 3, 63, 64, 65, 127, 128, 129} <= c                          # the 64-lane edges of ldc_finish's strided loops
    assert all({p - 1, p, p + 1} <= c for p in (32, 64, 128, 256, 512, 1024, 2048))   # P == count: no bitonic padding
    total = 10 * sum(K.LADDER_COUNTS)
    for cap in K.LADDER_CAPS:                                                # several filling passes, and cells larger than one pass
        assert total > cap and max(c) > cap
    assert sum(n > K.LADDER_CAPS[1] for n in c) >= 10 and sum(n > K.LADDER_CAPS[0] for n in c) >= 6
    assert any(n <= K.LDS_MAX < m for n, m in zip(K.LADDER_COUNTS, K.LADDER_COUNTS[1:]))   # LDS- and HBM-sized cells side by side


def test_count_ten_tells_a_float32_trim_from_a_double_one():
    assert int(F(10) * F(0.9)) == 9 and int(float(F(10)) * float(F(0.9))) == 8
    # and the ladder sees the difference: one more entry changes the curve's last values in the count-10 column
    fx = K.ladder(False)
    k = K.LADDER_COUNTS.index(10)
    pobs = np.sort(fx.pobs[np.nonzero((fx.px > k * K.LADDER_SPACING - 5000) & (fx.px < k * K.LADDER_SPACING + 5000))[0]])
    assert pobs.size == 10 and pobs[8] != pobs[7]
    _, tags, _, _ = fx.restate(0.1, 0.9)
    assert set(tags.reshape(fx.bg.shape)[:, k]) & {R.B3, R.B4}                # cells whose result depends on the last entry


def test_sub_ladders():
    below = K.ladder(True, K.ladder_columns(K.LDS_MAX))
    assert below.counts.max() == K.LDS_MAX and below.bg.shape == (10, 22)
    one = K.ladder(True, K.ladder_columns(K.LDS_MAX + 1), rows=(4,))
    assert (one.counts > K.LDS_MAX).sum() == 1 and one.bg.shape == (1, 23)   # the HBM kernel for a single cell
    full = K.ladder(True)
    for sub in (below, one):
        for q in ((0.0, 1.0), (0.1, 0.9)):
            np.testing.assert_array_equal(sub.restate(*q)[0].view(np.uint32), K.sub_grid(full.restate(*q)[0], sub).view(np.uint32))
    perm = K.ladder(True, permuted=True)
    assert not np.array_equal(perm.px, full.px) and np.array_equal(np.sort(perm.px), np.sort(full.px))


# ---- 2. zero rho ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.ZERO_RHO)
def test_zero_rho_cells(case):
    fx = K.zero_rho(case)
    out, tags, counts, sums = fx.restate()
    assert tags[0] == R.B4 and counts[0] == 10
    zero_r, zero_f = sums["sum_r"][0] == 0, sums["sum_f"][0] == 0
    assert (zero_r, zero_f) == {"ref": (True, False), "fcst": (False, True), "both": (True, True), "vertical": (True, True)}[case]
    assert (sums["sum_rho"][0] == 0) == (case in ("both", "vertical"))
    if case in ("both", "vertical"):
        assert sums["w0"][0] == 0
    else:
        assert 0 < sums["w0"][0] < 1
    assert np.isnan(out.ravel()[0])                                           # the project's rule for an undefined index
    assert np.isfinite(out.ravel()[1:]).all()
    rho = fx.cands[0][1]
    if case in ("ref", "fcst"):
        assert (rho[list(K._INSIDE)] == 0).all() and (np.delete(rho, K._INSIDE) > 0.7).all()
    else:
        assert rho.size == 10 and (rho == 0).all()
    if case == "vertical":
        assert fx.cv is None and fx.oracle_structure.cv == 0


# ---- 3. thresholds ------------------------------------------------------------------------------------------------------------------
def test_threshold_cells_take_the_derived_branches():
    fx = K.thresholds()
    out, tags, counts, _ = fx.restate()
    tags, counts = tags.reshape(fx.bg.shape), counts.reshape(fx.bg.shape)
    for k, name in enumerate(K.THRESHOLD_COLUMNS):
        assert tuple(tags[:, k]) == K.THRESHOLD_TAGS[name], (name, tags[:, k])
    valid = np.isfinite(fx.bg)
    np.testing.assert_array_equal(counts[valid], np.broadcast_to([12, 12, K.THRESHOLD_MIN_POINTS, K.THRESHOLD_MIN_POINTS - 1], fx.bg.shape)[valid])
    # the literals: float32(0.01) is below the double 0.01, float32(0.1) above the double 0.1, and one float step crosses each
    assert float(K.F001) < 0.01 < float(np.nextafter(K.F001, F(1))) and float(np.nextafter(K.F01, F(0))) < 0.1 < float(K.F01)
    assert np.signbit(fx.bg[4, 0]) and out[4, 0] == 0 and not np.signbit(out[4, 0])      # -0 -> branch 1 -> +0
    assert np.isposinf(out[5, 0]) and np.isnan(out[6, 0])
    assert out[2, 0] == K.F01 and out[3, 0] == 0
    assert F(3) * F(0.5) == fx.bg[0, 1] and out[0, 1] == F(1.5) and out[1, 1] == 0          # the 2a boundary
    assert fx.bg[0, 2] == fx.fcst_last and fx.fcst_last > 2                              # the branch-3 boundary
    few = K.THRESHOLD_COLUMNS.index("few")
    np.testing.assert_array_equal(out[:, few].view(np.uint32), fx.bg[:, few].view(np.uint32))
    assert np.signbit(out[5, few])                                                       # too few pairs: -0 stays -0


def test_threshold_values_at_their_places():
    fx = K.thresholds()
    w, S = fx.first["wet"], fx.px.size
    flat_o, flat_b = fx.pobs.ravel(), fx.pbg.ravel()
    assert np.isposinf(flat_b[2 * S + w + 1]) and flat_o[3 * S + w + 2] == -1 and np.isnan(flat_b[0 * S + w + 2])
    assert np.signbit(flat_o[1 * S + w]) and flat_o[1 * S + w] == 0 and np.signbit(flat_b[3 * S + w]) and flat_b[3 * S + w] == 0
    # read as (station, time) instead, the dropped entries would belong to other stations
    assert not np.isposinf(fx.pbg.T.ravel()[2 * S + w + 1])
    # a kept -0 keys as +0: with it the sorted ref values start 0, 0 (pobs[1, w] and the curve's own point)
    d = fx.first["dry"]
    assert np.signbit(fx.pobs[2, d + 1]) and fx.pbg[:, d:d + 3].max() == F(0.02) and fx.pbg[:, fx.first["half"]:fx.first["half"] + 3].max() == F(0.5)


# ---- 4. membership ------------------------------------------------------------------------------------------------------------------
def test_membership_at_exactly_the_localization_distance():
    fx = K.membership("Barnes")
    assert fx.oracle_structure.localization_distance() == 5000.0
    g, p = fx.oracle_points
    d = np.sqrt(p.x * p.x + p.y * p.y)
    assert list(d[:4]) == [5000.0] * 4 and d[4] < 5000 and d[5] > 5000
    # exactly R on a diagonal is in (d <= R); exactly R on an axis fails the open box (x < x0 + R); half a metre inside is in; the next
    # representable distance beyond R is out
    assert [list(idx) for idx, _ in fx.cands] == [[0, 1, 4], []]
    _, tags, counts, _ = fx.restate()
    assert list(counts) == [6, 0] and tags[0] == R.B4                        # T = 2: two pairs per kept station


def test_linear_structure_has_no_neighbours():
    fx = K.membership("Linear")
    assert fx.oracle_structure.localization_distance() == 0.0
    assert [list(idx) for idx, _ in fx.cands] == [[], []]
    out, tags, counts, _ = fx.restate()
    assert list(counts) == [0, 0] and list(tags) == [R.B2C, R.B2B]
    assert out[0, 0] == fx.bg[0, 0] and out[0, 1] == 0
