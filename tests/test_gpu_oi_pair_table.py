"""The pair table of the observation index (csrc/oi_pair_table.h) and its lookup in the P build of k_oi_union (csrc/oi_union.h), on the cases
of tests/oi_pair_table_cases.py (tests/test_oi_pair_table_cases_oracle.py checks their geometry on the CPU).  Every case runs three ways --
default, under GPP_OI_NO_PAIR_TABLE, under GPP_OI_PAIR_WINDOW=1 -- which must give THE SAME BITS and agree with the CPU oracle (RTOL 1e-5
over a floor of 1e-3, NaN pattern equal: the comparison of the parity tests).  No case can pass by falling back: the default run asserts a
table and no work item that evaluated, the window-1 run asserts items that did on the cases built for it."""
import numpy as np
import pytest

from tests import oi_pair_table_cases as T
from tests import oi_union_selection_cases as K
from tests.test_gpu_oi_union_bulk_cert import H, _check

pytestmark = pytest.mark.gpu


def _three(call, ref, misses_at_one=None):
    (out, out0, out1), (s, s0, s1) = T.three_ways(call)
    print(s, s0, s1, sep="\n")
    assert s["union_kernel_ms"] > 0, s
    assert s["pair_window"] > 0 and 0 < s["pair_table_bytes"] <= T.CAP and s["pair_fallback_items"] == 0, s
    assert s0["pair_window"] == 0 and s0["pair_table_bytes"] == 0 and s0["pair_fallback_items"] == 0 and s0["pair_table_build_ms"] == 0, s0
    assert s1["union_kernel_ms"] > 0 and s1["pair_window"] == 1, s1
    if misses_at_one:
        assert s1["pair_fallback_items"] > 0, s1
    if ref is not None:
        _check(out, ref)
    assert np.array_equal(out, out0, equal_nan=True) and np.array_equal(out, out1, equal_nan=True)
    return out, s


def _call(c, mp, st=None, handles=None, fresh_grid=True):
    """fresh_grid: every call on a NEW Grid of the case.  A Grid remembers how its last call with this Points and structure went, and a
    geometry whose tiles were mostly declined (a single declined tile) goes straight to k_oi the next time -- no tile kernel, no table:
    the three ways would not run the same path."""
    import gridpp_amd as gridpp
    grid, points = handles or T.handles(c)
    st = st or gridpp.BarnesStructure(*c["st"])

    def call():
        g = T.handles(c)[0] if fresh_grid else grid
        return gridpp.optimal_interpolation(g, c["bg"], points, c["obs"], c["ratios"], c["pbg"], st, mp)
    return call


@pytest.mark.parametrize("name", T.NAMES)
def test_case(name):
    _three(_call(T.build(name), T.mp_of(name)), T.oracle(name), name in T.WINDOW1_MISSES)


def test_one_points_through_four_keys():
    """h = 10 000, then 5 000, then an elevation factor, then another max_points: the table is rebuilt for every key (a build time is
    reported, the cached call after it reports none), every result equals its run without the table, and the first key once more as well"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = T.build("nan_elevation")
    handles = T.handles(c)
    og, op = T.opts(c)
    first = None
    # (the elevation factor with the case's own h: with h = 5 000 and v = 200 this geometry's cells agree on too little and the call goes to k_oi)
    for st, mp in (((10000.0,), 30), ((5000.0,), 30), ((H, 200.0), 30), ((10000.0,), 20), ((10000.0,), 30)):
        call = _call(c, mp, gridpp.BarnesStructure(*st), handles)
        call()
        built = gridpp.oi_last_stats()
        assert built["pair_window"] > 0 and built["pair_table_build_ms"] > 0, built          # (another key than the call before)
        ref = O.oi(og, c["bg"].ravel(), op, c["obs"], c["ratios"], c["pbg"], O.Barnes(*st), mp).reshape(c["bg"].shape)
        out, s = _three(call, ref)
        if first is None:
            first = out
    assert np.array_equal(out, first, equal_nan=True)


def _no_table(call, ref):
    import gridpp_amd as gridpp
    out = np.asarray(call())
    s = gridpp.oi_last_stats()
    assert s["pair_window"] == 0 and s["pair_table_bytes"] == 0 and s["pair_fallback_items"] == 0, s
    gridpp.set_path_override(T.NO_TABLE, "1")
    try:
        out0 = np.asarray(call())
    finally:
        gridpp.set_path_override(T.NO_TABLE, None)
    _check(out, ref)
    assert np.array_equal(out, out0, equal_nan=True)


def test_other_structures_take_no_table():
    """a Cressman structure and a spatially varying Barnes structure on the Points a Barnes call has built a table for"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c, mp = T.build(K.CRESSMAN), T.mp_of(K.CRESSMAN)
    handles = T.handles(c)
    grid = handles[0]
    _three(_call(c, mp, None, handles), T.oracle(K.CRESSMAN), True)
    og, op = T.opts(c)
    S = c["plat"].size
    ones_g, ones_p = np.ones(og.n, np.float32), np.ones(S, np.float32)
    st, ost = K.cressman()
    ref, _ = O.oi_full_generic(og, c["bg"].ravel(), ones_g, op, c["obs"], c["ratios"], c["pbg"], ones_p, ost, mp)
    _no_table(_call(c, mp, st, handles, fresh_grid=False), np.asarray(ref).reshape(c["bg"].shape))
    hf = (H * np.random.default_rng(5).uniform(0.8, 1.2, c["bg"].shape)).astype(np.float32)
    zf = np.zeros_like(hf)
    min_rho = O.Barnes(H).min_rho
    Rf = np.array([O.structure_localization("Barnes", h, min_rho) for h in hf.ravel()], np.float32)
    oi = O.nearest_indices(og, op)
    cell_p, obs_p = [hf.ravel(), zf.ravel(), zf.ravel(), Rf], [hf.ravel()[oi], zf.ravel()[oi], zf.ravel()[oi], Rf[oi]]
    ref, _ = O.oi_full_generic(og, c["bg"].ravel(), ones_g, op, c["obs"], c["ratios"], c["pbg"], ones_p, O.Struct("Barnes", H), mp, True, cell_p, obs_p)
    _no_table(_call(c, mp, gridpp.BarnesStructure(grid, hf, zf, zf, min_rho), handles, fresh_grid=False), np.asarray(ref).reshape(c["bg"].shape))


def test_cap_shrinks_the_window():
    """200 000 observations, one per (300 m)^2, around a 32 x 32 grid: the window the geometry asks for would take several hundred MiB"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    from tests.test_gpu_oi_union_bulk_cert import _latlon
    rng = np.random.default_rng(77)
    S, half = 200000, 0.5 * 300.0 * np.sqrt(200000.0)
    xs, ys = np.meshgrid(np.arange(32) * 100.0, np.arange(32) * 100.0)
    lats, lons = _latlon(xs, ys)
    plat, plon = _latlon(1600.0 + rng.uniform(-half, half, S), 1600.0 + rng.uniform(-half, half, S))
    bg = rng.normal(0, 1, (32, 32)).astype(np.float32)
    obs, pbg, ratios = rng.normal(0, 1, S).astype(np.float32), rng.normal(0, 1, S).astype(np.float32), rng.uniform(0.1, 1, S).astype(np.float32)
    grid, points, st = gridpp.Grid(lats, lons), gridpp.Points(plat, plon), gridpp.BarnesStructure(H)
    call = lambda: gridpp.optimal_interpolation(grid, bg, points, obs, ratios, pbg, st, 30)
    out = np.asarray(call())
    s = gridpp.oi_last_stats()
    print(s)
    assert s["union_kernel_ms"] > 0 and 0 < s["pair_window"] < 5 and T.CAP // 4 < s["pair_table_bytes"] <= T.CAP, s
    gridpp.set_path_override(T.NO_TABLE, "1")
    try:
        out0 = np.asarray(call())
    finally:
        gridpp.set_path_override(T.NO_TABLE, None)
    assert np.array_equal(out, out0, equal_nan=True)
    _check(out, O.oi(O.Pts(lats.ravel(), lons.ravel()), bg.ravel(), O.Pts(plat, plon), obs, ratios, pbg, O.Barnes(H), 30).reshape(32, 32))
