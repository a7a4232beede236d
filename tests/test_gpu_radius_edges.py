"""count, gridding (its three kernels), gridding_nearest, get_neighbours*, get_closest_neighbours, distance, nearest and the batched C entry
point on the device against the C oracle at the edges of gridpp_amd/csrc/radius.hip, radius_csr.h and the nearest kernels of runtime.hip.
The cases, their references and the proofs that they can tell a wrong kernel from a right one live in tests/radius_cases.py and
tests/test_radius_cases_oracle.py (no GPU).  Every comparison is bit for bit (NaN equals NaN) -- Mean and Sum too, since the values are
multiples of 0.25 whose float32 sums are exact in any order -- except Std / Variance (rtol 1e-5, atol 1e-5) and great-circle distances
(rtol 1e-5, atol 0.05), which keep the tolerances of tests/test_gpu_radius_parity.py.

Which kernel a call reaches:
  gridding, streaming statistic   k_radius_statistic_wave; GPP_GRIDDING_THREAD: k_radius_statistic; GPP_GRIDDING_CSR: k_radius_count,
                                  k_radius_fill, k_segment_statistic in passes of GPP_CSR_CAP entries
  gridding, Median                the CSR path always
  count, get_neighbours*          k_radius_count (+ k_radius_fill)
  distance                        k_knn_max_distance
  nearest, gridding_nearest       k_nearest_bruteforce up to 2048 points in the searched set (or GPP_NN_BRUTE), k_nearest_binned above
  an input set of 2^17 points     the index is built on the device unless GPP_HOST_INDEX"""
import ctypes as C
import functools

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

from tests import radius_cases as K

pytestmark = pytest.mark.gpu
F = np.float32
THREAD, CSR, CAP, BRUTE, HOST_INDEX = "GPP_GRIDDING_THREAD", "GPP_GRIDDING_CSR", "GPP_CSR_CAP", "GPP_NN_BRUTE", "GPP_HOST_INDEX"


def _gridpp():
    import gridpp_amd as gridpp
    return gridpp


@functools.lru_cache(maxsize=None)
def _ipoints(c):
    return _gridpp().Points(c.ilat, c.ilon, type=c.ctype)


@functools.lru_cache(maxsize=None)
def _opoints(c):
    return _gridpp().Points(c.olat, c.olon, type=c.ctype)


@functools.lru_cache(maxsize=None)
def _ogrid(c):
    shape = c.oshape or (1, c.olat.size)
    return _gridpp().Grid(c.olat.reshape(shape), c.olon.reshape(shape), type=c.ctype)


@functools.lru_cache(maxsize=None)
def _igrid(c):
    return _gridpp().Grid(c.ilat.reshape(c.ishape), c.ilon.reshape(c.ishape), type=c.ctype)


def _stat(name):
    return getattr(_gridpp(), name)


def _check_stat(out, ref, stat, msg=""):
    out = np.asarray(out).ravel()
    if stat in K.BITWISE:
        assert_array_equal(out, ref, err_msg="%s %s" % (stat, msg))
    else:
        assert_array_equal(np.isnan(out), np.isnan(ref), err_msg="%s %s" % (stat, msg))
        assert_allclose(out, ref, equal_nan=True, err_msg="%s %s" % (stat, msg), **K.SPREAD_TOL)


def _check_gridding(c, monkeypatch, stats=K.STATS, rows=None, as_grid=False):
    """every statistic on every (radius, min_num) row: the default kernel against the oracle, the other two bit-equal to it"""
    gridpp = _gridpp()
    out_set = _ogrid(c) if as_grid else _opoints(c)
    for radius, min_num in (rows or c.rows):
        for stat in stats:
            out = np.asarray(gridpp.gridding(out_set, _ipoints(c), c.values_for(stat), radius, min_num, _stat(stat)))
            assert out.shape == ((c.oshape or (1, c.olat.size)) if as_grid else (c.olat.size,))
            _check_stat(out, c.gridding(radius, min_num, stat), stat, "radius %g min_num %d" % (radius, min_num))
            if stat == "Median":
                continue
            for path in (THREAD, CSR):
                monkeypatch.setenv(path, "1")
                other = np.asarray(gridpp.gridding(out_set, _ipoints(c), c.values_for(stat), radius, min_num, _stat(stat)))
                monkeypatch.delenv(path)
                assert_array_equal(other, out, err_msg="%s %s radius %g min_num %d" % (path, stat, radius, min_num))


def _check_layout(c, points=None, device_built=False):
    """the index the device walks is the one tests/radius_cases.py restates: the bins and row segments claimed for a case are the ones visited"""
    lay = _gridpp().obs_index_layout(points if points is not None else _ipoints(c))
    ix = c.index
    assert _gridpp().obs_index_axes(points if points is not None else _ipoints(c)) == ix.axes
    assert (lay["nbx"], lay["nby"], lay["amin"], lay["bmin"], lay["inv_s"]) == (ix.nbx, ix.nby, ix.amin, ix.bmin, ix.inv_s)
    assert_array_equal(lay["bin_start"], ix.start)
    assert lay["device_built"] == device_built
    print("%s: axes %s, %d x %d bins of %.6g, fullest bin %d points, built on the %s"
          % (c.name, ix.axes, ix.nbx, ix.nby, ix.s, np.diff(ix.start).max(), "device" if device_built else "host"))


def _check_count(c):
    gridpp = _gridpp()
    for radius in sorted({r for r, _ in c.rows}):
        assert_array_equal(gridpp.count(_ipoints(c), _opoints(c), radius), c.count(radius), err_msg="radius %g" % radius)
        assert_array_equal(gridpp.count(_opoints(c), _ipoints(c), radius), c.count(radius, True), err_msg="reverse, radius %g" % radius)
        assert_array_equal(gridpp.count(_ipoints(c), _ogrid(c), radius).ravel(), c.count(radius), err_msg="to a Grid, radius %g" % radius)


def _check_neighbours(c, queries, radii):
    p = _ipoints(c)
    for q in queries:
        lat, lon = float(c.olat[q]), float(c.olon[q])
        for radius in radii:
            for inc in (True, False):
                ref = c.neighbours(q, radius, inc)
                msg = "query %d radius %g include_match %s" % (q, radius, inc)
                assert_array_equal(p.get_neighbours(lat, lon, radius, inc), ref, err_msg=msg)
                assert p.get_num_neighbours(lat, lon, radius, inc) == len(ref), msg
                idx, dist = p.get_neighbours_with_distance(lat, lon, radius, inc)
                assert_array_equal(idx, ref, err_msg=msg)
                assert_array_equal(dist, c.chord(q, ref), err_msg=msg)


def _check_knn(c, queries, nums, dist_nums=None):
    """get_closest_neighbours on single queries; distance in both argument orders; nearest"""
    gridpp = _gridpp()
    p = _ipoints(c)
    for q in queries:
        lat, lon = float(c.olat[q]), float(c.olon[q])
        for num in nums:
            for inc in (True, False):
                assert_array_equal(p.get_closest_neighbours(lat, lon, num, inc), c.closest(q, num, inc),
                                   err_msg="query %d num %d include_match %s" % (q, num, inc))
        for inc in (True, False):
            first = c.closest(q, 1, inc)
            assert p.get_nearest_neighbour(lat, lon, inc) == (first[0] if len(first) else -1)
    for num in (nums if dist_nums is None else dist_nums):
        for out, ref in ((gridpp.distance(p, _opoints(c), num), c.distance(num, True)),
                         (gridpp.distance(p, _ogrid(c), num).ravel(), c.distance(num, False))):
            if c.ctype == K.CARTESIAN:
                assert_array_equal(out, ref, err_msg="num %d" % num)
            else:
                assert_allclose(out, ref, err_msg="num %d" % num, **K.ARC_TOL)
    assert_array_equal(gridpp.nearest(p, _opoints(c), c.values), c.nearest())


# ---- 1. the boundary lattice ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("queries", ["nodes", "centres"])
@pytest.mark.parametrize("offset", K.LATTICE_OFFSETS)
def test_lattice_count(offset, queries):
    gridpp = _gridpp()
    c = K.lattice_case(offset, queries)
    _check_count(c)
    for radius in K.LATTICE_RADII + (float("inf"), float("nan"), -1.0):         # count does not validate its radius
        assert_array_equal(gridpp.count(_igrid(c), _ogrid(c), radius).ravel(), c.count(radius), err_msg="Grid to Grid, radius %g" % radius)
        assert_array_equal(gridpp.count(_igrid(c), _opoints(c), radius), c.count(radius), err_msg="Grid to Points, radius %g" % radius)
        assert_array_equal(gridpp.count(_ipoints(c), _opoints(c), radius), c.count(radius), err_msg="radius %g" % radius)
    if queries == "nodes":
        at = lambda r: gridpp.count(_ipoints(c), _opoints(c), r)[K.LATTICE_CENTRE]      # noqa: E731
        assert (at(5.0), at(1.0), at(0.0), at(10.0)) == (77, 1, 0, 313)


@pytest.mark.parametrize("as_grid", [False, True])
@pytest.mark.parametrize("queries", ["nodes", "centres"])
@pytest.mark.parametrize("offset", K.LATTICE_OFFSETS)
def test_lattice_gridding(offset, queries, as_grid, monkeypatch):
    c = K.lattice_case(offset, queries)
    _check_gridding(c, monkeypatch, as_grid=as_grid)
    if queries == "nodes":
        out = np.asarray(_gridpp().gridding(_opoints(c), _ipoints(c), np.ones(c.ilat.size, F), 5.0, 0, _stat("Sum")))
        assert out[K.LATTICE_CENTRE] == 77


def test_gridding_rejects_the_radii_count_takes():
    gridpp = _gridpp()
    c = K.lattice_case(0.0, "nodes")
    for radius in (float("inf"), float("nan"), -1.0):
        with pytest.raises(ValueError):
            gridpp.gridding(_opoints(c), _ipoints(c), c.values, radius, 0, gridpp.Mean)
    with pytest.raises(ValueError):
        gridpp.gridding(_opoints(c), _ipoints(c), c.values, 5.0, -1, gridpp.Mean)


@pytest.mark.parametrize("offset", K.LATTICE_OFFSETS)
def test_lattice_neighbours(offset):
    c = K.lattice_case(offset, "nodes")
    _check_neighbours(c, K.LATTICE_QUERIES, K.LATTICE_RADII)
    cc = K.lattice_case(offset, "centres")
    _check_neighbours(cc, (0, 9 * 20 + 9, 399), K.LATTICE_RADII + (0.5,))
    p = _ipoints(c)
    lat = lon = offset + 10.0
    assert [p.get_num_neighbours(lat, lon, r, inc) for r, inc in ((5, True), (5, False), (1, True), (1, False), (0, True))] == [77, 76, 1, 0, 0]
    g = _igrid(c)                                                               # the Grid forms of the same queries
    assert g.get_num_neighbours(lat, lon, 5.0) == 77 and g.get_num_neighbours(lat, lon, 5.0, False) == 76
    assert len(g.get_neighbours(lat, lon, 5.0)) == 77


# ---- 2. axis pairs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.AXIS_CASES))
def test_axis_pairs_radius_consumers(name, monkeypatch):
    c = K.axis_case(name)
    axes = _gridpp().obs_index_axes(_ipoints(c))
    assert axes == c.index.axes and (K.AXIS_CASES[name] is None or axes == K.AXIS_CASES[name])
    _check_layout(c)
    _check_count(c)
    _check_gridding(c, monkeypatch)
    _check_neighbours(c, (0, 5, 19, 20, 150, 298, 299), [r for r, _ in c.rows])


@pytest.mark.parametrize("name", sorted(K.AXIS_CASES))
def test_axis_pairs_nearest_consumers(name, monkeypatch):
    c = K.axis_case(name)
    assert _gridpp().obs_index_axes(_ipoints(c)) == c.index.axes
    _check_knn(c, (0, 19, 20, 150, 299), (1, 7), dist_nums=(1, 3, 40))
    _check_gridding_nearest(c, monkeypatch, ("Mean", "Count", "Median"))


def _check_gridding_nearest(c, monkeypatch, stats, min_nums=(0, 1, 3)):
    """input points and output locations swapped (more than 2048 locations: k_nearest_binned; GPP_NN_BRUTE: k_nearest_bruteforce)"""
    gridpp = _gridpp()
    for brute in (False, True):
        if brute:
            monkeypatch.setenv(BRUTE, "1")
        for stat in stats:
            for m in min_nums:
                out = gridpp.gridding_nearest(_ipoints(c), _opoints(c), _swapped_values(c), m, _stat(stat))
                assert_array_equal(out, _swapped(c).gridding_nearest(m, stat), err_msg="%s min_num %d brute %s" % (stat, m, brute))
    monkeypatch.delenv(BRUTE)


@functools.lru_cache(maxsize=None)
def _swapped(c):
    """the case with input set and output locations exchanged: its many points become the locations of gridding_nearest"""
    return K.Case(c.name + "-swapped", c.ctype, c.olat, c.olon, c.ilat, c.ilon, K.quarter_values(c.olat.size, 21, 9), [])


def _swapped_values(c):
    return _swapped(c).values


# ---- 3. chunk lengths ---------------------------------------------------------------------------------------------------------------
def test_chunk_lengths_on_all_three_kernels(monkeypatch):
    c = K.chunk_case()
    _check_layout(c)
    _check_count(c)
    _check_gridding(c, monkeypatch)
    _check_gridding(c, monkeypatch, stats=("Sum", "Std"), rows=[(1.0, n) for n in (63, 65, 66)], as_grid=True)


# ---- 4. degenerate and clamped geometry -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.DEGENERATE)
def test_degenerate_sets(name, monkeypatch):
    c = K.degenerate_case(name)
    if not c.index.tied_axes:                                                   # (tied extents: which axis comes second is the sort's choice)
        _check_layout(c)
    _check_count(c)
    _check_gridding(c, monkeypatch)
    radii = [r for r, _ in c.rows]
    _check_neighbours(c, tuple(range(0, 15, 2)) + tuple(K.DEGENERATE_FAR)[::3], radii)
    n = c.ilat.size
    _check_knn(c, (0, 4, 14, 15, 22), (1, min(n, 3), n + 1) if n < 10 else (1, 3), dist_nums=(1, 2, 5) if n < 10 else (1, 20))


# ---- 5. min_num and statistics ----------------------------------------------------------------------------------------------------
def test_min_num_and_special_lists(monkeypatch):
    gridpp = _gridpp()
    c = K.lists_case()
    _check_gridding(c, monkeypatch)
    _check_gridding(c, monkeypatch, as_grid=True)
    k = {n: i for i, n in enumerate(K.LIST_KINDS)}
    for stat in ("Std", "Variance"):
        out = np.asarray(gridpp.gridding(_opoints(c), _ipoints(c), c.values_for(stat), K.LIST_RADIUS, K.LIST_C, _stat(stat)))
        assert out[k["one_valid"]] == 0 and out[k["all_equal"]] == 0
    cnt = [np.asarray(gridpp.gridding(_opoints(c), _ipoints(c), c.values, K.LIST_RADIUS, m, gridpp.Count)) for m in K.LIST_MIN_NUMS]
    assert cnt[0][k["empty"]] == 0 and np.isnan(cnt[1][k["empty"]])
    assert cnt[2][k["ordinary"]] == 5 and np.isnan(cnt[3]).all()              # c >= min_num holds at c, fails at c + 1


@pytest.mark.parametrize("path", [None, THREAD, CSR])
def test_empty_input_and_empty_output(path, monkeypatch):
    gridpp = _gridpp()
    c = K.lists_case()
    if path:
        monkeypatch.setenv(path, "1")
    none = gridpp.Points([], [], type=K.CARTESIAN)
    nq = c.olat.size
    assert_array_equal(gridpp.count(none, _opoints(c), 10.0), np.zeros(nq, F))
    assert gridpp.count(_ipoints(c), none, 10.0).shape == (0,)
    for stat in K.STATS:
        for m in (0, 1):
            out = np.asarray(gridpp.gridding(_opoints(c), none, np.zeros(0, F), 10.0, m, _stat(stat)))
            want = 0.0 if (stat == "Count" and m == 0) else np.nan
            assert_array_equal(out, np.full(nq, want, F), err_msg="%s min_num %d" % (stat, m))
            assert_array_equal(out, K.Case("none", K.CARTESIAN, [], [], c.olat, c.olon, [], []).gridding(10.0, m, stat))
            assert np.asarray(gridpp.gridding(none, _ipoints(c), c.values, 10.0, m, _stat(stat))).shape == (0,)
            assert_array_equal(gridpp.gridding_nearest(_opoints(c), none, np.zeros(0, F), m, _stat(stat)), np.full(nq, np.nan, F))
    assert_array_equal(gridpp.distance(none, _opoints(c), 3), np.zeros(nq, F))
    assert len(none.get_neighbours(0.0, 0.0, 10.0)) == 0 and len(none.get_closest_neighbours(0.0, 0.0, 3)) == 0
    assert none.get_nearest_neighbour(0.0, 0.0) == -1 and none.get_num_neighbours(0.0, 0.0, 5.0) == 0


# ---- 6. paths -----------------------------------------------------------------------------------------------------------------------
def test_csr_cap_at_the_largest_list(monkeypatch):
    gridpp = _gridpp()
    c = K.chunk_case()
    for radius, min_num in ((1.0, 0), (200.0, 64)):
        largest = int(c.count(radius).max())
        for cap in (1, largest - 1, largest, largest + 1):
            monkeypatch.setenv(CAP, str(cap))
            out = np.asarray(gridpp.gridding(_opoints(c), _ipoints(c), c.values, radius, min_num, gridpp.Median))
            _check_stat(out, c.gridding(radius, min_num, "Median"), "Median", "cap %d radius %g" % (cap, radius))
            monkeypatch.setenv(CSR, "1")
            for stat in K.STREAMING:
                out = np.asarray(gridpp.gridding(_opoints(c), _ipoints(c), c.values_for(stat), radius, min_num, _stat(stat)))
                _check_stat(out, c.gridding(radius, min_num, stat), stat, "cap %d radius %g" % (cap, radius))
            monkeypatch.delenv(CSR)
    monkeypatch.delenv(CAP)


def test_device_built_index_against_host_built(monkeypatch):
    """2^17 + 3 points: the index of a fresh Points is built on the device, under GPP_HOST_INDEX on the host; it is cached per object"""
    gridpp = _gridpp()
    c = K.big_case()
    monkeypatch.setenv(HOST_INDEX, "1")
    host = gridpp.Points(c.ilat, c.ilon, type=c.ctype)
    _check_layout(c, host)                                                      # (builds it)
    monkeypatch.delenv(HOST_INDEX)
    dev = gridpp.Points(c.ilat, c.ilon, type=c.ctype)
    _check_layout(c, dev, device_built=True)
    op = _opoints(c)
    for radius, min_num in c.rows:
        outs = [gridpp.count(p, op, radius) for p in (host, dev)]
        assert_array_equal(outs[0], outs[1])
        assert_array_equal(outs[1], c.count(radius))
        for stat in K.STATS:
            outs = [np.asarray(gridpp.gridding(op, p, c.values_for(stat), radius, min_num, _stat(stat))) for p in (host, dev)]
            assert_array_equal(outs[0], outs[1], err_msg=stat)
            _check_stat(outs[1], c.gridding(radius, min_num, stat), stat, "radius %g" % radius)
    for q in (0, 19, 20, 200, 359):
        lat, lon = float(c.olat[q]), float(c.olon[q])
        for radius in (0.25, 300.0, 1500.0):
            ref = c.neighbours(q, radius, True)
            for p in (host, dev):
                idx, dist = p.get_neighbours_with_distance(lat, lon, radius)
                assert_array_equal(idx, ref)
                assert_array_equal(dist, c.chord(q, ref))
    for num in (1, 5):
        outs = [gridpp.distance(p, op, num) for p in (host, dev)]
        assert_array_equal(outs[0], outs[1])
        assert_array_equal(outs[1], c.distance(num, True))
    for p in (host, dev):
        assert_array_equal(gridpp.nearest(p, op, c.values), c.nearest())


# ---- 7. gridding_nearest ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("brute", [False, True])
@pytest.mark.parametrize("no", K.NEAREST_SIZES)
def test_gridding_nearest_sizes_and_ties(no, brute, monkeypatch):
    gridpp = _gridpp()
    if brute:
        monkeypatch.setenv(BRUTE, "1")
    for kind in ("ties", "one"):
        c = K.nearest_case(no, kind)
        largest = int(np.nanmax(c.gridding_nearest(0, "Count")))
        top = int(np.bincount(_o_targets(c)).max())
        for stat in K.STATS:
            for m in (0, 1, top, top + 1):
                out = gridpp.gridding_nearest(_opoints(c), _ipoints(c), c.values, m, _stat(stat))
                assert_array_equal(out, c.gridding_nearest(m, stat), err_msg="%s %s min_num %d" % (kind, stat, m))
        assert largest >= 1
        if no > 1:
            shape = (2, no // 2) if no % 2 == 0 else (1, no)
            grid = gridpp.Grid(c.olat.reshape(shape), c.olon.reshape(shape), type=c.ctype)
            out = np.asarray(gridpp.gridding_nearest(grid, _ipoints(c), c.values, 1, gridpp.Sum))
            assert out.shape == shape
            assert_array_equal(out.ravel(), c.gridding_nearest(1, "Sum"))
    # the indices behind it: nearest with ties
    c = K.nearest_case(no)
    assert_array_equal(_ipoints(c)._nearest_flat(c.olat, c.olon), _o_nearest_indices(c.ipts, c.opts))
    assert_array_equal(_opoints(c)._nearest_flat(c.ilat, c.ilon), _o_targets(c))


def _o_nearest_indices(g, q):
    from oracle import oracle as O
    return O.nearest_indices(g, q)


def _o_targets(c):
    """the location every input point goes to"""
    return _o_nearest_indices(c.opts, c.ipts)


def test_gridding_nearest_device_values_and_no_input():
    import torch
    gridpp = _gridpp()
    c = K.nearest_case(1025)
    out = gridpp.gridding_nearest(_opoints(c), _ipoints(c), torch.from_numpy(c.values).cuda(), 1, gridpp.Mean)
    assert out.is_cuda
    assert_array_equal(out.cpu().numpy(), c.gridding_nearest(1, "Mean"))
    none = gridpp.Points([], [], type=K.CARTESIAN)
    assert_array_equal(gridpp.gridding_nearest(_opoints(c), none, np.zeros(0, F), 0, gridpp.Count), np.full(1025, np.nan, F))


# ---- 8. k nearest -----------------------------------------------------------------------------------------------------------------
def test_knn_num_around_the_set_size_with_ties():
    c = K.knn_lattice_case()
    _check_knn(c, range(0, c.olat.size, 7), K.KNN_NUMS)
    g = _igrid(c)
    for q in (0, 40, 100):
        lat, lon = float(c.olat[q]), float(c.olon[q])
        for num in K.KNN_NUMS:
            assert_array_equal(g.get_closest_neighbours(lat, lon, num), np.stack(np.unravel_index(c.closest(q, num), c.ishape), 1)
                               if num else np.zeros((0, 2), int))
    for num in K.KNN_NUMS:
        assert_array_equal(_gridpp().distance(g, _ogrid(c), num).ravel(), c.distance(num, False))
        assert_array_equal(_gridpp().distance(g, _opoints(c), num), c.distance(num, True))


@pytest.mark.parametrize("dup", [1, 2, 7])
def test_duplicates_of_the_query(dup):
    c = K.duplicates_case(dup)
    p = _ipoints(c)
    lat, lon = float(c.olat[0]), float(c.olon[0])
    assert list(p.get_closest_neighbours(lat, lon, dup + 1)) == [4] + list(range(20, 20 + dup))
    rest = p.get_closest_neighbours(lat, lon, 30, False)
    assert len(rest) == 19 and 4 not in rest and rest.max() < 20
    _check_knn(c, (0, 1), (1, dup, dup + 1, dup + 2, 19, 20 + dup, 40))
    _check_neighbours(c, (0, 1), (0.125, 30.0, 1000.0))


@pytest.mark.parametrize("n", [300, 1100])
def test_far_clusters_ring_search(n):
    """the ring search crosses more than 95 empty rings (midpoint), or 200 (beside a cluster with num beyond it), up to rmax; 2 x 1100 points
    put nearest on k_nearest_binned"""
    c = K.clusters_case(n)
    _check_layout(c)
    nums = K.CLUSTER_NUMS if n == 300 else (1, 299)
    _check_knn(c, range(c.olat.size), nums)
    if n == 300:
        _check_knn(c, (0, 1), (n - 1, n, n + 1, 2 * n, 2 * n + 1), dist_nums=())


# ---- 9. the batched entry point ----------------------------------------------------------------------------------------------------
def _batch(p, qlat, qlon, radius, include_match, cap, indices=True, distances=True, offsets=True):
    from gridpp_amd import _capi
    nq = len(qlat)
    qlat, qlon = np.ascontiguousarray(qlat, F), np.ascontiguousarray(qlon, F)
    counts = np.full(max(nq, 1), K.SENTINEL_I, np.int32)
    off = np.full(nq + 1, K.SENTINEL_I, np.int64)
    idx = np.full(max(cap, 1) + 8, K.SENTINEL_I, np.int32)
    dist = np.full(max(cap, 1) + 8, K.SENTINEL_F, F)
    total = C.c_longlong(-5)
    ptr = lambda a, on=True: C.c_void_p(a.ctypes.data) if on else None          # noqa: E731
    rc = _capi.lib().gpp_points_get_neighbours_batch(p._h, ptr(qlat), ptr(qlon), nq, float(radius), int(include_match), ptr(counts),
                                                     ptr(off, offsets), ptr(idx, indices), ptr(dist, distances), cap, C.byref(total))
    assert rc == 0
    return counts[:nq], off, idx, dist, total.value


@pytest.mark.parametrize("include_match", [True, False])
def test_batch_entry_point(include_match):
    c, q, _, _, _, _ = K.batch_case()
    lists = [c.neighbours(int(k), K.BATCH_RADIUS, include_match) for k in q]
    counts = np.array([len(l) for l in lists], np.int32)
    offsets = np.concatenate(([0], np.cumsum(counts)))
    ref_idx = np.concatenate(lists)
    ref_dist = np.concatenate([c.chord(int(k), l) for k, l in zip(q, lists)])
    total = int(counts.sum())
    assert total > counts.max() > 0
    p = _ipoints(c)
    qlat, qlon = c.olat[q], c.olon[q]
    untouched_i, untouched_f = np.full(total + 8, K.SENTINEL_I, np.int32), np.full(total + 8, K.SENTINEL_F, F)
    # cap too small: counts, offsets and the total only
    cnt, off, idx, dist, tot = _batch(p, qlat, qlon, K.BATCH_RADIUS, include_match, total - 1)
    assert_array_equal(cnt, counts)
    assert_array_equal(off, offsets)
    assert tot == total
    assert_array_equal(idx, untouched_i[:-1])
    assert_array_equal(dist, untouched_f[:-1])
    # cap == total, all four forms of the payload
    for want_i, want_d, want_o in ((True, True, True), (True, False, True), (False, True, True), (True, True, False), (False, False, True)):
        cnt, off, idx, dist, tot = _batch(p, qlat, qlon, K.BATCH_RADIUS, include_match, total, want_i, want_d, want_o)
        assert_array_equal(cnt, counts)
        assert tot == total
        assert_array_equal(off, offsets if want_o else np.full(len(q) + 1, K.SENTINEL_I))
        assert_array_equal(idx[:total], ref_idx if want_i else untouched_i[:total])
        assert_array_equal(dist[:total], ref_dist if want_d else untouched_f[:total])
        assert_array_equal(idx[total:], untouched_i[total:])                    # nothing beyond the payload
        assert_array_equal(dist[total:], untouched_f[total:])
    # no query, no neighbour at all, an empty set
    cnt, off, idx, dist, tot = _batch(p, qlat[:0], qlon[:0], K.BATCH_RADIUS, include_match, 10)
    assert tot == 0 and (idx == K.SENTINEL_I).all() and (off == K.SENTINEL_I).all()
    cnt, off, idx, dist, tot = _batch(p, qlat, qlon, 0.0, include_match, 10)
    assert tot == 0 and (cnt == 0).all() and (off == 0).all() and (idx == K.SENTINEL_I).all() and (dist == K.SENTINEL_F).all()
    none = _gridpp().Points([], [], type=K.CARTESIAN)
    cnt, off, idx, dist, tot = _batch(none, qlat, qlon, K.BATCH_RADIUS, include_match, 10)
    assert tot == 0 and (cnt == 0).all() and (off == 0).all() and (idx == K.SENTINEL_I).all()
    cnt, off, idx, dist, tot = _batch(none, qlat, qlon, K.BATCH_RADIUS, include_match, 10, offsets=False)
    assert tot == 0 and (cnt == 0).all() and (off == K.SENTINEL_I).all()
