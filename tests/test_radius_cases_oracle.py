"""The cases of tests/radius_cases.py can tell a wrong radius-query kernel from a right one (no GPU): the oracle gives the hand-derived counts
on the boundary lattice, a closed-box or open-disc restatement of the membership test differs on every boundary case, every tie case has
two candidates at bit-equal float32 distance, and the numpy restatement of the index build shows that the axis-pair, chunk-length, clamp
and ring-search cases reach what they claim."""
import numpy as np
import pytest

from tests import radius_cases as K

F = np.float32
C = K.LATTICE_CENTRE


def _counts(case, q, radius):
    return [len(K.members(case, q, radius, **kw)) for kw in ({}, {"closed_box": True}, {"open_disc": True})]


# ---- 1. boundary lattice ----------------------------------------------------------------------------------------------------------
def test_oracle_on_the_hand_derived_lattice_counts():
    c = K.lattice_case(0.0, "nodes")
    assert len(c.neighbours(C, 5.0, True)) == 77 and len(c.neighbours(C, 5.0, False)) == 76
    assert len(c.neighbours(C, 1.0, True)) == 1 and len(c.neighbours(C, 1.0, False)) == 0
    assert len(c.neighbours(C, 0.0, True)) == 0 and len(c.neighbours(C, 0.0, False)) == 0
    assert c.count(5.0)[C] == 77 and c.count(1.0)[C] == 1 and c.count(0.0)[C] == 0
    assert c.count(10.0)[C] == 317 - 4                                      # the closed disc of radius 10 without its four axis nodes
    d = c.chord(C, np.arange(c.ipts.n))
    dx, dy = c.ipts.x - c.opts.x[C], c.ipts.y - c.opts.y[C]
    on_circle = d == 5
    on_axis = on_circle & ((dx == 0) | (dy == 0))
    assert on_circle.sum() == 12 and on_axis.sum() == 4
    kept = np.zeros(c.ipts.n, bool)
    kept[c.neighbours(C, 5.0, True)] = True
    assert (kept & on_circle).sum() == 8 and not (kept & on_axis).any()       # the 3-4-5 nodes stay, the box drops the axis nodes
    assert (d <= 5).sum() == 81 and (d < 5).sum() == 69


@pytest.mark.parametrize("offset", K.LATTICE_OFFSETS)
def test_wrong_comparisons_differ_on_the_lattice(offset):
    c = K.lattice_case(offset, "nodes")
    assert _counts(c, C, 5.0) == [77, 81, 69]
    assert _counts(c, C, 10.0) == [313, 317, 305]
    assert _counts(c, C, 1.0) == [1, 5, 1]                                     # the box alone decides at radius 1
    assert len(set(_counts(c, 0, 13.0))) == 3                                  # from a corner: 5-12-13 on the circle, (0, 13) on the box
    for r in K.LATTICE_RADII:                                                  # the restatement is the oracle's test
        for inc in (True, False):
            assert np.array_equal(K.members(c, C, r, inc), c.neighbours(C, r, inc)), (r, inc)
    for q in K.LATTICE_QUERIES:                                                # corners and edges: the boundary is met everywhere
        assert len(set(_counts(c, q, 5.0))) == 3
    cc = K.lattice_case(offset, "centres")
    q = 9 * 20 + 9
    # from a cell centre nothing lies on the box; (0.5, 2.5)-(1.5, 2.5) style pairs put nodes on circles of half-integer squares only
    assert len(K.members(cc, q, 0.5)) == 0 and len(K.members(cc, q, 1.0)) == 4
    for r in K.LATTICE_RADII:
        assert np.array_equal(K.members(cc, q, r), cc.neighbours(q, r, True))


def test_one_float_step_around_five():
    below, above = K.LATTICE_RADII[2], K.LATTICE_RADII[4]
    assert F(below) < F(5) < F(above) and np.nextafter(F(below), F(9)) == F(5) and np.nextafter(F(5), F(9)) == F(above)
    c = K.lattice_case(0.0, "nodes")
    # one step below: the open disc.  One step above: 10 - r is exact and lets the two low axis nodes in, 10 + r = 15 + 2^-21 is a tie between
    # 15 and 15 + 2^-20 and rounds to the even 15, so the two high axis nodes stay on the box: 81 - 2
    assert c.count(below)[C] == 69 and c.count(above)[C] == 79
    big = K.lattice_case(float(2 ** 22), "nodes")                              # there x -+ radius rounds to the node itself
    assert big.count(below)[C] == 69 and big.count(above)[C] == 77


def test_count_takes_any_radius():
    c = K.lattice_case(0.0, "nodes")
    assert (c.count(float("inf")) == 441).all() and (c.count(float("nan")) == 0).all() and (c.count(-1.0) == 0).all()


# ---- 2. axis pairs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.AXIS_CASES))
def test_axis_pairs(name):
    c = K.axis_case(name)
    want = K.AXIS_CASES[name]
    if want:
        assert c.index.axes == want and not c.index.tied_axes
    assert c.index.nbx > 8 and c.index.nby > 8
    cnt = c.count(c.rows[1][0])
    assert cnt.max() > 3 and (cnt == 0).any() and (c.count(c.rows[0][0])[:20] >= 1).all()
    assert (c.count(c.rows[2][0]) > 500).any()


# ---- 3. chunk lengths ---------------------------------------------------------------------------------------------------------------
def test_chunk_case_reaches_every_length():
    c = K.chunk_case()
    ix = c.index
    assert ix.axes == (0, 1)
    for k, L in enumerate(K.CHUNK_LENGTHS):
        segs = ix.segments(K.query3(c, k), 1.0)
        assert segs == [L], (k, segs)                                          # one row, one segment, exactly the cluster
        m = ix.segment_members(K.query3(c, k), 1.0)[0]
        hit = np.isin(m, c.neighbours(k, 1.0, True))
        assert hit[:64].all()                                                  # the first chunk is full (as far as it goes)
        if L > 64:
            rest = hit[64:]
            assert rest[0] and (rest.size == 1 or rest.sum() < rest.size)      # the others are sparse, lane 0 of the second one hits
            assert np.isnan(c.values[m[64]])
        assert np.isnan(c.values[m[0]]) and (L < 64 or np.isnan(c.values[m[63]]))
        assert c.count(1.0)[k] == hit.sum() == (L if L <= 64 else 64 + len(range(64, L, 5)))
    # the wide radius joins several bins per row and several rows
    wide = [ix.segments(K.query3(c, k), K.CHUNK_RADII[1]) for k in range(len(K.CHUNK_LENGTHS))]
    assert all(len(s) >= 3 for s in wide) and any(max(s) >= 129 for s in wide)
    bx0, bx1, _, _ = ix.box(K.query3(c, 3), K.CHUNK_RADII[1])
    assert bx1 - bx0 >= 3


# ---- 4. degenerate and clamped geometry -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.DEGENERATE)
def test_degenerate_cases_clamp(name):
    c = K.degenerate_case(name)
    ix = c.index
    if name in ("one", "coincident500", "geo_one"):
        assert ix.s <= 2e-3 and abs(1.0 / float(ix.inv_s) - ix.s) < 1e-6        # extents floored at 1e-3
    if name.startswith("line_"):
        assert 1 in (ix.nbx, ix.nby) and max(ix.nbx, ix.nby) > 100
    small, reach, cover = (r for r, _ in c.rows)
    clamped = 0
    for q in K.DEGENERATE_FAR:
        bx0, bx1, by0, by1 = ix.box(K.query3(c, q), small)
        assert (bx0 == bx1 and bx0 in (0, ix.nbx - 1)) or (by0 == by1 and by0 in (0, ix.nby - 1))
        clamped += (bx0 == bx1) + (by0 == by1)
        assert c.count(small)[q] == 0
    assert clamped >= 8
    assert (c.count(reach)[list(K.DEGENERATE_FAR)] > 0).any() and (c.count(cover) == c.ipts.n).all()
    # the near queries sit on the smallest and the largest coordinate of the binned axes
    a, b = ix.axes
    qa, qb = (c.opts.x, c.opts.y, c.opts.z)[a][:15], (c.opts.x, c.opts.y, c.opts.z)[b][:15]
    assert (qa == ix.amin).any() and (qb == ix.bmin).any() and (qa == ix.amax).any() and (qb == ix.bmax).any()
    assert ix.bin_a(ix.amax) == ix.nbx - 1 or ix.amax == ix.amin


# ---- 5. min_num ---------------------------------------------------------------------------------------------------------------------
def test_lists_case_counts():
    c = K.lists_case()
    cnt = c.count(K.LIST_RADIUS)
    assert list(cnt) == [K.LIST_C] * (len(K.LIST_KINDS) - 1) + [0]
    k = {n: i for i, n in enumerate(K.LIST_KINDS)}
    for stat in ("Std", "Variance"):
        out = c.gridding(K.LIST_RADIUS, K.LIST_C, stat)
        assert out[k["one_valid"]] == 0 and out[k["all_equal"]] == 0 and np.isnan(out[k["all_nan"]]) and np.isnan(out[k["mixed_inf"]])
    assert c.gridding(K.LIST_RADIUS, 0, "Count")[k["empty"]] == 0 and np.isnan(c.gridding(K.LIST_RADIUS, 1, "Count")[k["empty"]])
    assert np.isnan(c.gridding(K.LIST_RADIUS, 0, "Mean")[k["empty"]])
    assert c.gridding(K.LIST_RADIUS, K.LIST_C, "Count")[k["ordinary"]] == 5 and np.isnan(c.gridding(K.LIST_RADIUS, K.LIST_C + 1, "Count")).all()
    assert c.gridding(K.LIST_RADIUS, K.LIST_C, "Count")[k["all_pinf"]] == 0


# ---- 6. the large set ------------------------------------------------------------------------------------------------------------
def test_big_case_is_above_the_device_index_threshold():
    c = K.big_case()
    assert c.ipts.n == (1 << 17) + 3 and c.opts.n <= 400
    cnt = c.count(1500.0)
    assert 40 < cnt.max() < 300 and (cnt == 0).any() and (c.count(0.25)[:20] >= 1).all()


# ---- 7. gridding_nearest ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no", K.NEAREST_SIZES)
def test_nearest_cases_hold_ties(no):
    c = K.nearest_case(no)
    ncand = np.array([len(K.tie_candidates(c, i)) for i in range(c.ipts.n)])
    if no >= 64:
        assert (ncand == 2).any() and (ncand == 4).any() and (ncand == 1).any()
    elif no == 2:
        assert (ncand == 2).any()
    received = np.nan_to_num(c.gridding_nearest(0, "Count"), nan=0)        # (Count counts the valid values)
    assert received.sum() == np.isfinite(c.values).sum()
    if no >= 1024:
        assert (received == 0).any()                                          # locations that receive nothing
    # a last-tie rule would move points: the lowest candidate is the oracle's target
    bits = 1
    while (1 << bits) < no:
        bits += 1
    assert (1 << bits) >= no and (bits == 1 or (1 << (bits - 1)) < no)
    one = K.nearest_case(no, "one")
    got = np.nan_to_num(one.gridding_nearest(0, "Count"), nan=0)
    assert got[no // 2] == np.isfinite(one.values).sum() == got.sum()


# ---- 8. k nearest -----------------------------------------------------------------------------------------------------------------
def test_knn_lattice_has_ties_at_the_cut():
    c = K.knn_lattice_case()
    p, o = c.ipts, c.opts
    tied = 0
    for q in range(o.n):
        s2 = (p.x - o.x[q]) ** 2 + (p.y - o.y[q]) ** 2
        s2.sort()
        tied += s2[0] == s2[1]
    assert tied > o.n // 2                                                     # the nearest point itself is tied for most queries
    assert np.array_equal(c.closest(0, K.KNN_N + 1), c.closest(0, K.KNN_N)) and len(c.closest(0, 0)) == 0


@pytest.mark.parametrize("dup", [1, 2, 7])
def test_duplicates_case(dup):
    c = K.duplicates_case(dup)
    first = list(c.closest(0, dup + 1))
    assert first == [4] + list(range(20, 20 + dup))                             # the point and its copies, by index
    rest = c.closest(0, 30, False)
    assert len(rest) == 19 and 4 not in rest and rest.max() < 20
    assert _o_nearest(c, 0, False) == rest[0] and _o_nearest(c, 0, True) == 4


def _o_nearest(c, q, inc):
    from oracle import oracle as O
    return O.nearest_neighbour(c.ipts, float(c.olat[q]), float(c.olon[q]), inc)


@pytest.mark.parametrize("n", [300, 1100])
def test_clusters_lie_200_bins_apart(n):
    c = K.clusters_case(n)
    ix = c.index
    assert ix.axes == (0, 1) and ix.nbx > 200 and ix.nby <= 2               # (Cartesian: x is the second coordinate)
    b = ix.bin_a(c.ipts.x)
    assert b[n:].min() - b[:n].max() >= 200
    mid = int(ix.bin_a(c.opts.x[0]))
    assert mid - b[:n].max() > 95 and b[n:].min() - mid > 95                 # empty rings on both sides of the midpoint
    assert (c.ipts.n > 2048) == (n == 1100)
    # num beyond the near cluster: the farthest neighbour of the query beside cluster 0 lies in cluster 1
    assert c.closest(1, n + 1).max() >= n and c.closest(1, n - 1).max() < n


# ---- 9. batch ----------------------------------------------------------------------------------------------------------------------
def test_batch_case():
    c, q, counts, offsets, idx, dist = K.batch_case()
    assert counts[2] == 77 and offsets[-1] == counts.sum() == idx.size == dist.size
    assert (dist <= K.BATCH_RADIUS).all() and (dist == 5).sum() >= 8
    assert K.SENTINEL_I not in idx and K.SENTINEL_F not in dist
