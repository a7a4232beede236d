"""The reference side of the gridops edge suite (tests/test_gpu_gridops_edges.py), without a GPU: the cases of tests/gridops_cases.py
can tell a wrong kernel from a right one (a scan that lets the last of equal values win gives other answers on most cells; exact
counts, ranges and radii do occur), and the oracle gives the hand-derived answers at the new shapes."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import gridops_cases as K


# ---- fill_missing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, field, expected", K.fill_missing_known_answers(), ids=[k[0] for k in K.fill_missing_known_answers()])
def test_fill_missing_known_answers(name, field, expected):
    from oracle import oracle as O
    assert K.segment_length(max(field.shape)) == 3          # 600 elements: the runs span many three-element segments
    assert_array_equal(O.fill_missing(field), expected)


def test_fill_missing_cases_follow_their_patterns():
    assert len(set(K.FM_CASES)) == len(K.FM_PATTERNS) * len(K.FM_SHAPES) and set(K.FM_DEVICE_CASES) <= set(K.FM_CASES)
    assert sorted(c.split("-")[0] for c in K.FM_DEVICE_CASES) == sorted(K.FM_PATTERNS)
    assert {K.segment_length(max(s)) for s in K.FM_SHAPES if max(s) <= K.FM_MAXX} == {1, 2, 3, 4, 32}
    for name in K.FM_CASES:
        pattern, shape = name.split("-")
        v = K.fill_missing_case(name)
        Y, X = v.shape
        assert "%dx%d" % (Y, X) == shape
        lines = v if X >= Y else v.T                       # the pattern runs along the longer axis
        n, seg, ok = lines.shape[1], K.segment_length(lines.shape[1]), np.isfinite(lines)
        if pattern == "random30":
            assert 0.2 < 1 - ok.mean() < 0.4
        elif pattern == "long_run":
            assert not ok[:, 10:n - 9].any() and ok[:, :10].all() and ok[:, n - 9:].all() and n - 19 > seg
        elif pattern == "leading_run":
            assert not ok[:, :n // 3 + 1].any() and ok[:, -1].all()
        elif pattern == "trailing_run":
            assert not ok[:, n - n // 3 - 1:].any() and ok[:, 0].all()
        elif pattern == "missing_line":
            assert not ok[0].any() and ok[1:].any()
        elif pattern == "single_valid":
            assert (ok.sum(1) == 1).all() and ok[0, 0] and ok[1, n // 2] and (len(ok) < 3 or ok[2, n - 1])
        elif pattern == "segment_starts":
            assert (np.flatnonzero(ok[0]) % seg == 0).all() and ok[0].sum() == -(-n // seg)
            assert ok[1].sum() == -(-n // (2 * seg))       # every other thread owns an empty segment
        elif pattern == "segment_ends":
            assert (np.flatnonzero(ok[0]) % seg == seg - 1).all() and ok[0].sum() == n // seg
        elif pattern == "inf_mixed":
            assert np.isposinf(lines).mean() > 0.05 and np.isneginf(lines).mean() > 0.05 and np.isnan(lines).mean() > 0.05
            assert np.isposinf(v[0, 0])


def test_fill_missing_oracle_treats_inf_as_missing():
    """the same field with every inf replaced by NaN has the same answer"""
    for name in ("inf_mixed-3x257", "inf_mixed-2x8192"):
        from oracle import oracle as O
        v = K.fill_missing_case(name)
        assert_array_equal(K.fill_missing_reference(name), O.fill_missing(np.where(np.isinf(v), K.NAN, v)))
        assert np.isfinite(K.fill_missing_reference(name)).mean() > 0.9


# ---- calc_gradient --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["hw1", "hw2"])
def test_minmax_case_tells_first_tie_from_last(row):
    share = K.differing_share(K.minmax_reference(row), K.minmax_last_tie_wins(row))
    print("MinMax %s: a last-tie-wins scan differs on %.2f of the cells" % (row, share))
    assert share >= 0.5


def _minmax_window_facts(hw):
    """(count, range) of every window of the tie case, by numpy: range = max - min of base over the valid cells (NaN: none)"""
    base, values = K.minmax_tie_case()
    ok = K.finite(base) & K.finite(values)
    Y, X = base.shape
    rng = np.full((Y, X), np.nan)
    for y in range(Y):
        for x in range(X):
            w = (slice(max(0, y - hw), y + hw + 1), slice(max(0, x - hw), x + hw + 1))
            b = base[w][ok[w]]
            if b.size:
                rng[y, x] = b.max() - b.min()
    return K.window_count(ok, hw), rng


def test_minmax_counts_sit_on_num_min():
    count, _ = _minmax_window_facts(1)
    Y, X = K.GRAD_SHAPE
    corners = np.array([count[0, 0], count[0, X - 1], count[Y - 1, 0], count[Y - 1, X - 1]])
    edges = np.concatenate([count[0, 1:-1], count[-1, 1:-1], count[1:-1, 0], count[1:-1, -1]])
    assert (corners == 4).any() and (corners == 3).any()           # num_min 4: exactly met, and missed by one
    assert (edges == 6).any() and (edges == 5).any()               # num_min 6
    for row, num_min in (("count4", 4), ("count6", 6)):
        ref = K.minmax_reference(row)
        dflt = np.float32(K.MINMAX_ROWS[row][3])
        assert (ref[count < num_min] == dflt).all() and (ref[count == num_min] != dflt).mean() > 0.5


@pytest.mark.parametrize("row", ["range3", "range5"])
def test_minmax_range_sits_on_min_range(row):
    hw, num_min, min_range, dflt = K.MINMAX_ROWS[row]
    _, rng = _minmax_window_facts(hw)
    ref = K.minmax_reference(row)
    on = rng == min_range
    assert on.sum() > 100 and (row == "range5" or (rng > min_range).sum() > 100)
    assert (ref[on] == np.float32(dflt)).all()                     # `<= min_range`: the default
    assert (ref[rng > min_range] != np.float32(dflt)).all()


def test_minmax_whole_field_window_gives_one_value():
    ref = K.minmax_reference("hw50")
    assert np.unique(ref).size == 1 and ref[0, 0] != np.float32(K.MINMAX_ROWS["hw50"][3])


def test_linreg_constant_block_takes_the_default():
    base, values = K.linreg_case()
    assert (base[K.BLOCK] == 3.0).all() and K.finite(values[K.BLOCK]).all()
    for row in ("block_hw2", "block_hw2_range"):
        ref = K.linreg_reference(row)
        assert_array_equal(ref[K.BLOCK_INNER], np.full_like(ref[K.BLOCK_INNER], K.LINREG_DEFAULT))   # variance exactly 0
        assert (ref != np.float32(K.LINREG_DEFAULT)).mean() > 0.5


def test_linreg_whole_field_window_gives_one_value():
    ref = K.linreg_reference("hw60")
    assert np.unique(ref).size == 1 and ref[0, 0] != np.float32(K.LINREG_DEFAULT) and np.isfinite(ref[0, 0])


def test_linreg_counts_sit_on_num_min():
    base, values = K.linreg_case()
    count = K.window_count(K.finite(base) & K.finite(values), 1)
    dflt = np.float32(K.LINREG_DEFAULT)
    for row, num_min in (("count9", 9), ("count6", 6), ("count4", 4)):
        ref = K.linreg_reference(row)
        assert (count == num_min).sum() > 0 and (count == num_min - 1).sum() > 0
        assert (ref[count < num_min] == dflt).all()
        if row != "count4":                                        # (count4 also asks for a range)
            outside_block = np.ones(base.shape, bool)
            outside_block[K.BLOCK] = False
            assert (ref[(count == num_min) & outside_block] != dflt).all()
    assert count[0, 0] == 4 and K.linreg_reference("count4")[0, 0] != dflt


# ---- neighbourhood_search -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["nearest_ties", "point_target", "whole_field"])
def test_search_case_tells_first_tie_from_last(row):
    share = K.differing_share(K.search_reference(row, False), K.search_last_tie_wins(row))
    print("neighbourhood_search %s: a last-tie-wins scan differs on %.2f of the cells" % (row, share))
    assert share >= 0.2


def test_search_halfwidth_0_returns_the_array():
    array, search, apply = K.search_case()
    for with_apply in (False, True):
        ref = K.search_reference("hw0", with_apply)
        ok = K.finite(array)
        assert_array_equal(ref[ok], array[ok])
        assert_array_equal(ref, array)                             # (and the missing cells stay what they were)


def test_search_mixed_row_has_both_branches():
    array, search, apply = K.search_case()
    hw, tmin, tmax, delta = K.SEARCH_ROWS["mixed"]
    inrange = K.finite(search) & K.finite(array) & (search >= np.float32(tmin)) & (search <= np.float32(tmax))
    has = K.window_count(inrange, hw) > 0
    assert 0.2 < has[K.finite(search)].mean() < 0.98               # means of in-range cells and nearest targets both occur
    ref, ref_apply = K.search_reference("mixed", False), K.search_reference("mixed", True)
    assert K.differing_share(ref, array) > 0.5
    assert_array_equal(ref_apply[apply != 1], array[apply != 1])
    assert_array_equal(ref_apply[apply == 1], ref[apply == 1])
    assert sorted(np.unique(apply)) == [0, 1, 2]


# ---- fill, doping ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.expected_hits()))
def test_oracle_hit_sets(name):
    c = K.scatter_cases()[name]
    want = K.expected_hits()[name]
    for op in ("fill_in", "fill_out", "circle"):
        assert K.hit_set(name, K.scatter_reference(name, op), op) == want, op
    bg = K.background(c["grid"])
    ref = K.scatter_reference(name, "fill_out")
    assert (ref.ravel()[want] == bg.ravel()[want]).all() and (np.delete(ref.ravel(), want) == np.float32(K.FILL_VALUE)).all()
    if "square" in c["ops"]:
        assert_array_equal(K.scatter_reference(name, "square"), bg)


def test_radii_sit_on_the_boundaries():
    assert np.float32(1000.0) ** 2 * 2 == np.float32(2e6) and float(K.R_DIAGONAL) ** 2 > 2e6 > float(np.nextafter(K.R_DIAGONAL, np.float32(0))) ** 2
    lats, lons, elev, ct = K.grid_arrays("cart")
    assert ct == K.CARTESIAN and lats[10, 12] == 0 and lons[10, 12] == 0 and lats[3, 20] == -7000 and lons[3, 20] == 8000 and lats.shape == (K.CART_Y, K.CART_X)
    up = np.nextafter(np.float32(1000), np.float32(np.inf))
    assert np.float32(0) - up < -1000 and np.float32(8000) + up == 9000 and np.float32(-7000) + up == -6000    # exact at the origin only


@pytest.mark.parametrize("name", ["far_reaching", "near_outside", "geo_mixed"])
def test_clamped_points_still_reach_the_grid(name):
    c = K.scatter_cases()[name]
    hit = K.hit_set(name, K.scatter_reference(name, "fill_in"), "fill_in")
    assert 0.03 < len(hit) / K.background(c["grid"]).size < 0.97
    if name != "geo_mixed":                                         # every one of the eight outside points is the winner somewhere
        assert len(np.unique(K.scatter_reference(name, "circle"))) >= 8


def test_elevation_rule_hand_placed_cells():
    bg = K.background("cart")
    circle, square = K.scatter_reference("elev_circle", "circle"), K.scatter_reference("elev_square", "square")
    for out in (circle, square):
        assert out[4, 4] == 7 and out[4, 5] == 8                    # NaN point elevation; NaN point meets NaN cell
        assert out[15, 21] == 10 and out[0, 0] == 11                # valid point elevation, NaN cell
        assert out[16, 21] == bg[16, 21]                            # |100 - 470| > 50
        assert out[10, 12] == 12                                    # |250 - 300| == 50 is not `>`
    assert circle[15, 20] == 9 and square[15, 20] == 10             # (the square of point 3 reaches it too)
    assert circle[9, 12] == bg[9, 12] and circle[3, 4] == 7
    assert K.hit_set("elev_circle", circle, "circle") == sorted(
        [K.node(4, 4), K.node(3, 4), K.node(5, 4), K.node(4, 3), K.node(4, 5), K.node(4, 6), K.node(3, 6), K.node(5, 6), K.node(4, 7),
         K.node(15, 19), K.node(14, 19), K.node(16, 19), K.node(15, 18), K.node(15, 20), K.node(15, 21), K.node(0, 0), K.node(1, 0), K.node(0, 1),
         K.node(10, 12)])


def test_elevation_difference_of_zero():
    for name, op in (("elev_zero_circle", "circle"), ("elev_zero_square", "square")):
        c = K.scatter_cases()[name]
        assert c["med"] == 0.0 and c["elev"][0] == 300 and c["elev"][1] > 300 and c["elev"][1] - np.float32(300) == np.spacing(np.float32(300))
        assert K.hit_set(name, K.scatter_reference(name, op), op) == [K.node(10, 12)]
        assert K.scatter_reference(name, op)[10, 12] == 7


def test_doping_square_known_answers():
    bg = K.background("cart")
    out = K.scatter_reference("square_hw0", "square")
    assert K.hit_set("square_hw0", out, "square") == [K.node(2, 7), K.node(10, 12)] and out[10, 12] == 0 and out[2, 7] == 1
    assert_array_equal(K.scatter_reference("square_covers_all", "square"), np.zeros_like(bg))
    out = K.scatter_reference("square_huge_hw", "square")
    assert_array_equal(out, np.ones_like(bg))                       # the second point's window is everything
    out = K.scatter_reference("square_shared_cell", "square")
    want = bg.copy()
    want[8:13, 10:15] = 0
    want[9:12, 11:14] = 1                                           # same nearest node (10, 12): the higher index wins where both reach
    want[2, 7] = 2
    assert_array_equal(out, want)
    out = K.scatter_reference("square_outside", "square")
    want = bg.copy()                                                # nearest nodes: (0, 10), (19, 14), (7, 0), (12, 24) and the four corners
    want[0:3, 8:13], want[17:20, 12:17], want[5:10, 0:3], want[10:15, 22:25] = 0, 1, 2, 3
    want[0:4, 0:4], want[0:4, 21:25], want[16:20, 0:4], want[16:20, 21:25] = 4, 5, 6, 7
    assert_array_equal(out, want)
    far = K.scatter_reference("square_far_outside", "square")
    assert sorted(np.unique(far[far != bg])) == list(range(8))      # clipped at every edge and corner
