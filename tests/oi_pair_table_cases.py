"""Cases for the pair table of the observation index (csrc/oi_pair_table.h, the lookup in the P build of k_oi_union): the single tiles and
the 16 x 16 grid of tests/oi_union_selection_cases.py and tests/oi_union_split_cases.py, plus three of its own.  Shared by
tests/test_gpu_oi_pair_table.py and tests/test_oi_pair_table_cases_oracle.py, which checks on the CPU what the GPU test relies on:

  * default window: every two observations that any cell of the grid selects lie within the window of each other, so NO work item can
    miss (the GPU test asserts pair_fallback_items == 0);
  * window 1 (GPP_OI_PAIR_WINDOW=1), cases of WINDOW1_MISSES: EVERY updating cell selects two observations more than one bin row or column
    apart -- every work item has such a pair in its union, so every item that builds a P MUST miss (the GPU test asserts pair_fallback_items > 0).

The window and the bins are restated from csrc/oi.hip (pair_window_for, gpp_scan_geometry) and tests/radius_cases.py (Index)."""
import functools

import numpy as np

from tests import oi_union_selection_cases as K
from tests.test_gpu_oi_union_bulk_cert import DX, H, _latlon, _tile_case

NO_TABLE, WINDOW = "GPP_OI_NO_PAIR_TABLE", "GPP_OI_PAIR_WINDOW"
CAP = 128 << 20


def laf_factor():
    """land-fraction factor (w = 0.5) beside the elevation factor (v = 200 m): the table carries both"""
    c = _tile_case(38, [], seed=41, st=(H, 200.0, 0.5))
    rng = np.random.default_rng(141)
    c["elevs"], c["pelevs"] = rng.uniform(0, 300, c["bg"].shape).astype(np.float32), rng.uniform(0, 300, 38).astype(np.float32)
    c["lafs"], c["plafs"] = rng.uniform(0, 1, c["bg"].shape).astype(np.float32), rng.uniform(0, 1, 38).astype(np.float32)
    c["plafs"][[2, 9]] = np.nan
    return c


def one_bin():
    """34 observations within 60 m of the tile centre and one 1.9 km away: most of the cluster falls into one bin of the index"""
    c = _tile_case(34, [], seed=42, rmax=60.0)
    far = _tile_case(1, [], seed=43, rmin=1900.0, rmax=1900.0)
    rng = np.random.default_rng(142)
    c["plat"], c["plon"] = np.append(c["plat"], far["plat"]), np.append(c["plon"], far["plon"])
    c["obs"], c["pbg"] = rng.normal(0, 1, 35).astype(np.float32), rng.normal(0, 1, 35).astype(np.float32)
    c["ratios"] = rng.uniform(0.1, 1, 35).astype(np.float32)
    return c


def three_one_bin():
    """three observations whose extents east and north are equal: the index is ONE bin"""
    c = _tile_case(3, [], seed=44)
    c["plat"], c["plon"] = _latlon(np.array([-100.0, 900.0, -100.0]), np.array([-100.0, -100.0, 900.0]))
    return c


# name -> (builder, max_points); the K cases keep their names
OWN = {"laf_factor": (laf_factor, 30), "one_bin": (one_bin, 32), "three_one_bin": (three_one_bin, 30)}
FROM_K = ["mp8", "evict_35", "mp32", "form48", "form64", "grid16",      # 8 x 8 and 16 x 16, 35 .. 62 observations, max_points 8, 30, 32, 40, 50
          "ties2_first_pass",                                           # two observations at one place
          "u1", "u2", "u11",                                            # S = 1, 2, S < max_points
          "nan_elevation",                                              # NaN observation elevation, v = 200
          "evict_45", "u40"]                                            # a declined tile (16- and 4-cell items on the list passes); a 40-row union
NAMES = FROM_K + sorted(OWN)
# (not mp8: some of its cells select eight observations that span one bin -- an item of such cells need not miss)
WINDOW1_MISSES = ["evict_35", "mp32", "form48", "form64", "grid16", "evict_45", "u40", "nan_elevation", "laf_factor"]


@functools.lru_cache(maxsize=None)
def build(name):
    c = OWN[name][0]() if name in OWN else K.build(name)
    c = dict(c)
    c.setdefault("lafs", None); c.setdefault("plafs", None)
    return c


def mp_of(name):
    return OWN[name][1] if name in OWN else K.mp_of(name)


def opts(c):
    from oracle import oracle as O
    ge = None if c["elevs"] is None else c["elevs"].ravel()
    gl = None if c["lafs"] is None else c["lafs"].ravel()
    return O.Pts(c["lats"].ravel(), c["lons"].ravel(), ge, gl), O.Pts(c["plat"], c["plon"], c["pelevs"], c["plafs"])


@functools.lru_cache(maxsize=None)
def oracle(name):
    from oracle import oracle as O
    c = build(name)
    og, op = opts(c)
    out = O.oi(og, c["bg"].ravel(), op, c["obs"], c["ratios"], c["pbg"], O.Barnes(*c["st"]), mp_of(name)).reshape(c["bg"].shape)
    out.setflags(write=False)
    return out


def handles(c):
    import gridpp_amd as gridpp
    g = [a for a in (c["elevs"], c["lafs"]) if a is not None]
    p = [a for a in (c["pelevs"], c["plafs"]) if a is not None]
    return gridpp.Grid(c["lats"], c["lons"], *g), gridpp.Points(c["plat"], c["plon"], *p)


def three_ways(call):
    """call() three times: default, without the table, with a window of one bin -> ((out, out0, out1), (stats, stats0, stats1))"""
    import gridpp_amd as gridpp
    assert not {NO_TABLE, WINDOW} & set(gridpp.active_overrides())
    outs, stats = [np.asarray(call())], [gridpp.oi_last_stats()]
    for name, value in ((NO_TABLE, "1"), (WINDOW, "1")):
        gridpp.set_path_override(name, value)
        try:
            assert name in gridpp.active_overrides()
            outs.append(np.asarray(call())); stats.append(gridpp.oi_last_stats())
        finally:
            gridpp.set_path_override(name, None)
    return tuple(outs), tuple(stats)


# ---- the index and the window, restated ------------------------------------------------------------------------------------------------------
def window_asked(c, mp, ix):
    """pair_window_for: ceil((2 * 1.5 r_k + diagonal of a tile) / bin width), the tile 8 x 8 cells of DX metres"""
    occ = ix.S / float(ix.nbx * ix.nby)
    assert 0 < mp <= 62                                   # (then gpp_scan_geometry's kk is max_points itself)
    r_k = np.sqrt(mp / (np.pi * max(occ, 1e-3))) / float(ix.inv_s)
    return int(np.ceil((2.0 * float(np.float32(1.5 * r_k)) + 8 * DX * np.sqrt(2.0)) * float(ix.inv_s)))


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(window asked for, window in use, largest bin distance between two observations some cell / any two cells select, observations in
    the fullest bin, whether a selected observation sits in a corner bin of the index, the smallest such bin distance within one cell's selection)"""
    from oracle import oracle as O
    from tests.radius_cases import Index
    c, mp = build(name), mp_of(name)
    og, op = opts(c)
    ix = Index(op)
    bx, by = ix.bin % ix.nbx, ix.bin // ix.nbx
    st = O.Barnes(*c["st"])
    per_cell, least, union = 0, 1 << 30, set()
    for cell, b in enumerate(c["bg"].ravel()):
        if not np.isfinite(b):
            continue
        sel, _ = O.oi_selection(og, cell, op, c["obs"], c["pbg"], st, mp)
        sel = np.asarray(sel, np.int64)
        union |= set(sel.tolist())
        if sel.size:
            span = max(int(np.ptp(bx[sel])), int(np.ptp(by[sel])))
            per_cell, least = max(per_cell, span), min(least, span)
    u = np.array(sorted(union), np.int64)
    whole = max(int(np.ptp(bx[u])), int(np.ptp(by[u])))
    corner = bool((np.isin(bx[u], (0, ix.nbx - 1)) & np.isin(by[u], (0, ix.nby - 1))).any())
    asked = window_asked(c, mp, ix)
    return asked, min(asked, max(ix.nbx, ix.nby)), per_cell, whole, int(np.bincount(ix.bin).max()), corner, least
