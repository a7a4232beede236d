"""Single tiles (and one 16 x 16 grid) for the selection machinery of k_oi_union's scan (csrc/oi_union.h: worst_slot and its
minima without NaN handling, the eviction path of run_chunk, end_bulk) and for the triangle-index table of its P build.  Geometry and helpers of
tests/test_gpu_oi_union_bulk_cert.py: 8 x 8 cells 100 m apart, BarnesStructure(1000), R = 3 645 m; the observations of `evict` lie within 2 km
of the tile centre, so EVERY cell can use EVERY observation and a cell with more of them than max_points has to choose -- the bulk disc
takes the max_points records nearest to the tile centre, every later ring candidate a cell wants evicts that cell's worst entry.

Shared by tests/test_gpu_oi_union_selection.py, tests/test_oi_union_selection_cases_oracle.py (what each case claims, checked on the CPU with
the oracle) and tools/make_oi_union_selection_golden.py (the parent commit's bits of exactly these cases).

CASES: name -> (builder, max_points, claim).  claim = (cells with more usable observations than max_points, cells whose cut falls inside a
group of equal float32 rho, largest such group or 0), all three checked by the CPU test.  A tile whose selections together hold more than
40 observations cannot be solved by one shared factorisation of the 32-column form: it goes to the list passes, whose 16- and 4-cell items
run the same scan.  Which way each case was declined was read once from a GPP_UNION_STATS build (profiles/oi_union_selection_ab.txt) and is
not asserted -- the statistics of a product build do not tell the reasons apart: the scan itself declined for want of slots (alloc == FULL
after live_mask() had recycled) in evict_45, evict_60, evict_60b, mp31, mp32, partial_tile, nan_elevation, ties2, ties3 and four tiles of
grid16; "union > 40" was the reason in none (the slots run out first); evict_35, evict_40, mp8, mp9, mp16 and the two _first_pass tie
cases passed the scan and were declined for more than twelve extras; the others stay on the first pass.  Ties are made by observations at
one place, not by mirrored ones, and whether the tied slots sit in one group of eight or in two is not controlled.  A NaN cell or
observation COORDINATE is no case: Grid and Points refuse it (tests/test_oi_union_selection_cases_oracle.py).  Which slot a candidate lands in is the kernel's
business (bulk order, then the lowest free slot, recycled once all 40 are allocated): the cases reach the five slot groups by their
number of evicting candidates -- with max_points 30 the bulk fills slots 0..29, ring candidates take 30..39 and the evictions clear slots
anywhere in 0..39; with 15 or more ring candidates all 40 slots have been allocated and live_mask() recycles."""
import functools

import numpy as np

from tests import oi_union_split_cases as SPLIT
from tests.test_gpu_oi_union_bulk_cert import H, LEFT, OVERRIDE, _oracle, _side, _tile_case

RTOL = 1e-5


def evict(n, seed, **kw):
    return lambda: _tile_case(n, [], seed=seed, **kw)


def ties(n, groups, seed):
    """observations sharing one place: equal rho in every cell, different observation indices.  groups: tuples of observation indices; the
    first of each keeps its place, the others move onto it.  (Their rows of P are equal; R keeps P + R regular: ratios >= 0.1.)"""
    def build():
        c = _tile_case(n, [], seed=seed)
        for g in groups:
            for k in g[1:]:
                c["plat"][k], c["plon"][k] = c["plat"][g[0]], c["plon"][g[0]]
        return c
    return build


def store_and_evict():
    """28 observations every cell reaches and eight from the west that reach the first 1, 1, 2, 2, 3, 3, 4, 4 columns: column 0 has 36 usable
    observations and evicts, column 3 has exactly 30, columns 4..7 stay at 28 < max_points and only store"""
    return _tile_case(28, _side(LEFT, [0, 0, 1, 1, 2, 2, 3, 3]), seed=21)


def one_cell():
    return _tile_case(45, [], nan_cells=[(x, y) for y in range(8) for x in range(8) if (x, y) != (2, 6)], seed=22)


def nan_elevation():
    """elevation factor (v = 200 m); four observations and three cells without an elevation: their factor is 1 (the NaN is dropped)"""
    c = _tile_case(45, [], seed=23, st=(H, 200.0))
    rng = np.random.default_rng(123)
    c["elevs"], c["pelevs"] = rng.uniform(0, 300, c["bg"].shape).astype(np.float32), rng.uniform(0, 300, 45).astype(np.float32)
    c["pelevs"][[3, 17, 30, 44]] = np.nan
    c["elevs"][1, 2] = c["elevs"][5, 5] = c["elevs"][7, 0] = np.nan
    return c


def split(name):
    return lambda: dict(SPLIT.build(name), st=(H,), elevs=None, pelevs=None)


CASES = {
    # evictions, max_points 30: 5, 15 and 30 observations beyond the bulk disc
    "evict_35": (evict(35, 1), 30, (64, 0, 0)),
    "evict_45": (evict(45, 2), 30, (64, 0, 0)),
    "evict_60": (evict(60, 3), 30, (64, 0, 0)),
    "evict_60b": (evict(60, 4, rmax=1200.0), 30, (64, 0, 0)),
    # max_points at the group boundaries; groups that stay empty
    "mp1": (evict(40, 5), 1, (64, 0, 0)),
    "mp2": (evict(40, 6), 2, (64, 0, 0)),
    "mp8": (evict(40, 7), 8, (64, 0, 0)),
    "mp9": (evict(40, 8), 9, (64, 0, 0)),
    "mp31": (evict(45, 9), 31, (64, 0, 0)),
    "mp32": (evict(45, 10), 32, (64, 0, 0)),
    # equal rho at the cut: pairs and triples of observations at one place
    "ties2": (ties(48, [(0, 40), (5, 6), (11, 30), (17, 18), (23, 47), (29, 3), (35, 36), (41, 9)], 11), 30, (64, 7, 2)),
    "ties3": (ties(50, [(0, 25, 49), (7, 8, 9), (13, 31, 44), (19, 2, 38), (27, 28, 46)], 12), 30, (64, 14, 3)),
    "ties2_first_pass": (ties(39, [(0, 30), (5, 6), (11, 38), (17, 18), (23, 2), (29, 3), (35, 36)], 26), 30, (64, 7, 2)),
    "ties3_first_pass": (ties(40, [(0, 25, 39), (7, 8, 9), (13, 31, 34), (19, 2, 38), (27, 28, 16)], 27), 30, (64, 20, 3)),
    "evict_40": (evict(40, 28), 30, (64, 0, 0)),
    "store_and_evict": (store_and_evict, 30, (24, 0, 0)),
    "partial_tile": (evict(45, 13, ny=5, nx=11, nan_cells=((10, 4), (0, 2))), 30, (53, 0, 0)),
    "one_cell": (one_cell, 30, (1, 0, 0)),
    "mp16": (evict(60, 14, rmax=2400.0), 16, (64, 0, 0)),
    # the P build: unions of 1, 2, 11, 12, 32, 33 and 40 rows (no cell has to choose)
    "u1": (evict(1, 15), 32, (0, 0, 0)),
    "u2": (evict(2, 16), 32, (0, 0, 0)),
    "u11": (evict(11, 17), 32, (0, 0, 0)),
    "u12": (evict(12, 18), 32, (0, 0, 0)),
    "u32": (evict(32, 19), 32, (0, 0, 0)),
    "u33": (split("c28_e5"), 32, (0, 0, 0)),
    "u40": (split("c28_e12"), 32, (0, 0, 0)),
    # the wider forms
    "form48": (evict(52, 20), 40, (64, 0, 0)),
    "form64": (evict(62, 24), 50, (64, 0, 0)),
    "nan_elevation": (nan_elevation, 30, (64, 0, 0)),
    "grid16": (evict(55, 25, ny=16, nx=16, rmax=1800.0), 30, (256, 0, 0)),
}
CRESSMAN = "evict_45"                               # this case also runs with CressmanStructure(R): the generic instantiation
DECLINED_UNION = 40                                 # rows the shared factorisation of the 32-column form holds


@functools.lru_cache(maxsize=None)
def build(name):
    return CASES[name][0]()


def mp_of(name):
    return CASES[name][1]


@functools.lru_cache(maxsize=None)
def facts(name):
    """from the oracle: (cells with more usable observations than max_points, cells whose selection has a tie at the cut, the largest
    number of observations with the float32 rho of a cell's cut, the size of the union of all selections)"""
    from oracle import oracle as O
    c, mp = build(name), mp_of(name)
    st = O.Barnes(*c["st"])
    ge = None if c["elevs"] is None else c["elevs"].ravel()
    og, op = O.Pts(c["lats"].ravel(), c["lons"].ravel(), ge), O.Pts(c["plat"], c["plon"], c["pelevs"])
    more = tied = biggest = 0
    union = set()
    for cell, b in enumerate(c["bg"].ravel()):
        if not np.isfinite(b):
            continue
        rho = np.array([np.float32(st.corr((og.x[cell], og.y[cell], og.z[cell], og.elevs[cell], og.lafs[cell]), (op.x[k], op.y[k], op.z[k], op.elevs[k], op.lafs[k])))
                        for k in range(op.n)], np.float32)
        usable = np.nonzero(rho > 0)[0]
        more += usable.size > mp
        sel, tie = O.oi_selection(og, cell, op, c["obs"], c["pbg"], st, mp)
        union |= set(sel.tolist())
        if usable.size > mp:
            srt = np.sort(rho[usable])[::-1]
            if srt[mp - 1] == srt[mp]:       # the cut falls inside a group of equal rho
                tied += 1
                biggest = max(biggest, int((rho[usable] == srt[mp]).sum()))
                # ties go to the lower observation index (oi.cpp:262-273): the selected members of the group are its lowest indices
                grp = usable[rho[usable] == srt[mp]]
                inside = [k for k in grp if k in set(sel.tolist())]
                assert inside == sorted(grp.tolist())[:len(inside)], (name, cell)
    return more, tied, biggest, len(union)


def cressman():
    import gridpp_amd as gridpp
    from oracle import oracle as O
    R = float(np.float32(O.Barnes(H).localization_distance()))
    return gridpp.CressmanStructure(R), O.Struct("Cressman", R)


def run(name, structure=None):
    """the call, and the same call under GPP_OI_NO_BULK_CERT (the other form of the bulk loop): -> (analysis, analysis under the override, statistics)"""
    import gridpp_amd as gridpp
    c, mp = build(name), mp_of(name)
    if c["elevs"] is None:
        grid, points = gridpp.Grid(c["lats"], c["lons"]), gridpp.Points(c["plat"], c["plon"])
    else:
        grid, points = gridpp.Grid(c["lats"], c["lons"], c["elevs"]), gridpp.Points(c["plat"], c["plon"], c["pelevs"])
    st = structure if structure is not None else gridpp.BarnesStructure(*c["st"])
    assert OVERRIDE not in gridpp.active_overrides()
    out = np.asarray(gridpp.optimal_interpolation(grid, c["bg"], points, c["obs"], c["ratios"], c["pbg"], st, mp))
    s = gridpp.oi_last_stats()
    gridpp.set_path_override(OVERRIDE, "1")
    try:
        out0 = np.asarray(gridpp.optimal_interpolation(grid, c["bg"], points, c["obs"], c["ratios"], c["pbg"], st, mp))
        s0 = gridpp.oi_last_stats()
    finally:
        gridpp.set_path_override(OVERRIDE, None)
    assert s0["bulk_certified"] == 0, s0
    return out, out0, s


def oracle(name):
    return _oracle(build(name), mp_of(name))


def record():
    """every array of tests/golden/oi_union_selection_parent.npz"""
    rec = {}
    for name in sorted(CASES):
        out, out0, s = run(name)
        assert s["union_kernel_ms"] > 0, (name, s)
        assert np.array_equal(out, out0, equal_nan=True), name
        rec[name] = out
    out, out0, s = run(CRESSMAN, cressman()[0])
    assert s["union_kernel_ms"] > 0 and np.array_equal(out, out0, equal_nan=True), s
    rec["cressman_" + CRESSMAN] = out
    return rec
