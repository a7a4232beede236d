"""Single tiles for the split-row form of k_oi_union's shared factorisation (csrc/oi_union.h, GPP_UNION_SPLIT): every row of the union in two
lanes, columns 0..17 in the lower one and 18..31 in the upper one.  The tiles are built like those of tests/test_gpu_oi_union_solve.py (whose
helpers are used as they are) with a prescribed core size c and extras count nE; `build` asserts the (c, nE, largest extras count of a cell) a
case was made for.  Shared by tests/test_gpu_oi_union_split_rows.py, tests/test_oi_union_split_cases_oracle.py (the constructions, on the CPU)
and tools/make_oi_union_split_rows_golden.py (the parent's bits of exactly these cases).

What the form cannot be given, and why the list of cases stops where it does: with max_points <= 32 a cell holds c + (its extras) <= 32
observations, so c = 32 has no extras; and a union has at most twelve extras, so late columns (u > 32) exist from c = 21 on only -- the
chain of a late column always continues into the upper half (the kernel asserts 32 - 12 >= 18).  The late-column cases therefore have
c = 21 (three columns of the chain behind the hand-over), 24, 27, 28 and 31 (the largest core that has extras)."""
import numpy as np

from tests.test_gpu_oi_union_solve import (BOTTOM, CORNERS, H, LEFT, RIGHT, TOP, _E1, _E5, _E5_ONE, _E5_ONE_NAN, _E12, _E12_SIDES, _radius, _selections,
                                           _side, _tile_case, _union)

MP = 32
_E6 = _side(LEFT, [0, 1, 2]) + _side(RIGHT, [0, 1, 2])
# c of the core-only tiles: the slot alignment at 3 / 4, the hand-over of the pivots at 17 / 18 / 19, the headline's 28, every column
CORE_ONLY = (1, 3, 4, 5, 17, 18, 19, 28, 32)
# name -> (c, extras, cells without a background, (nE, largest extras count of a cell))
TILES = {
    "c12_e12": (12, _E12, (), (12, 6)),                        # core wholly in the lower half, extras rows 12 .. 23 reach into the upper one
    "c17_e6": (17, _E6, (), (6, 3)),                           # c = 4 k + 1 below 18: the padded reads of the finish meet columns 18, 19 of row 17
    "c18_e1": (18, _E1, (), (1, 1)),
    "c19_e1": (19, _E1, (), (1, 1)),
    "c19_e12": (19, _E12, (), (12, 6)),
    "c21_e12": (21, _E12, (), (12, 6)),                        # u = 33: one late column, its chain ends three columns behind the hand-over
    "c24_e12": (24, _E12, (), (12, 6)),                        # u = 36, even c
    "c27_e12": (27, _E12_SIDES, CORNERS, (12, 3)),             # u = 39: lane 61 idle, lane 62 live
    "c28_e12": (28, _E12_SIDES, CORNERS, (12, 3)),             # u = 40: all 64 lanes, eight late columns
    "c28_e5": (28, _E5, (), (5, 3)),                           # u = 33
    "c31_e5": (31, _E5_ONE, _E5_ONE_NAN, (5, 1)),              # u = 36: the longest chain a late column can have
    "c19_holes": (19, _E1, ((1, 0), (3, 2), (4, 4), (6, 5), (2, 7)), (1, 1)),   # cells without a background: `upd` has holes
}
for _c in CORE_ONLY:
    TILES["c%d" % _c] = (_c, [], (), (0, 0))
WITH_VARIANCE = ("c12_e12", "c19_e1", "c28_e12")


def build(name):
    c, extras, nan_cells, (nE, mmax) = TILES[name]
    case = _tile_case(c, extras, nan_cells, seed=700 + sum(map(ord, name)))
    assert _union(_selections(case, MP)) == (c, nE, 0, mmax), name
    return case


def one_cell():
    """a tile with ONE updating cell: its 19 observations are the core"""
    case = _tile_case(19, [], [(x, y) for y in range(8) for x in range(8) if (x, y) != (5, 3)], seed=41)
    assert _union(_selections(case, MP)) == (19, 0, 0, 0)
    return case


def extreme_cases():
    """allow_extrapolation = False: c = 28 core-only, and each of the 28 observations in turn carries by far the largest obs - background --
    whatever order the rows take, ten of the 28 calls have the extreme in a row >= 18"""
    base = build("c28")
    out = []
    for k in range(28):
        c = dict(base)
        c["obs"] = base["obs"].copy()
        c["obs"][k] = base["pbg"][k] + np.float32(6.0)
        out.append(c)
    return out


def negative_cases():
    """c = 19, observation k with ratio -5: the diagonal entry 1 - 5 of its row stays negative through the elimination, whatever order the
    rows take -- every row is the one with the non-positive pivot once, row 18 (an upper lane's) among them.  P + R is not singular: the
    call is redone by k_oi's pivoted LU and has a result."""
    out = []
    for k in range(19):
        c = _tile_case(19, [], seed=91)
        c["ratios"][k] = -5.0
        assert _union(_selections(c, MP)) == (19, 0, 0, 0)
        out.append(c)
    return out


def ending(case):
    """how a call ends: (1.0, NaNs) when the library raises `singular`, (0.0, analysis) otherwise"""
    try:
        return np.float32(0.0), run(case)[0]
    except RuntimeError as e:
        assert "singular" in str(e), e
        return np.float32(1.0), np.full(case["bg"].shape, np.nan, np.float32)


def pivot_cases():
    """c = 19, observations k and k + 1 (cyclically) at one place with ratio 0, as test_non_positive_pivot builds its pair: the later row of
    the two meets the pivot a - (a / sqrt(a))^2, a the pivot of the earlier one -- 0 when a is 1 or the rounding falls that way, else a
    few ulps to either side, so a pair may raise (k_oi's pivoted LU meets the same zero) or pass with whatever the tiny pivot gives.
    Either way the call ends as it did before the split.  Over the 19 pairs the row of that pivot is 18 for the two pairs that hold the
    observation of row 18 and below 18 for the seventeen others, whatever order the rows take."""
    out = []
    for k in range(19):
        c = _tile_case(19, [], seed=90)
        j = (k + 1) % 19
        for key in ("plat", "plon"):
            c[key][j] = c[key][k]
        c["ratios"][[k, j]] = 0.0
        assert _union(_selections(c, MP)) == (19, 0, 0, 0)
        out.append(c)
    return out


# ---- the list passes -----------------------------------------------------------------------------------------------------------------------
def list_case():
    """Fourteen observations every cell reaches; ten from the south that reach row 0 (three of them row 1 too) and one from the west that
    reaches column 0.  Cell (0, 0) has eleven extras: the tile is declined.  A short list of declined tiles goes straight to the sixteen
    4-cell items of each (k_oi_union<., true>, level 3), halves of a row: in row 0 all ten are core, c = 24 (pivots in the upper half), in
    row 1 three are, c = 17, in rows 2 .. 7 none, c = 14; the left halves have the one extra.  (16-cell items -- pairs of rows: 0-1 would
    be declined again with c = 17 and seven extras in a cell, the others solved with c = 14 -- are made of lists too long for that pass only, among at
    least as many tiles that are not declined: not a handful of tiles.  They run the same code under another lane mask.)"""
    case = _tile_case(14, _side(BOTTOM, [0, 0, 0, 0, 0, 0, 0, 1, 1, 1], spread=0.7) + _side(LEFT, [0]), seed=63)
    sel = _selections(case, MP)
    assert _union(sel) == (14, 11, 0, 11)
    rows = lambda y0, y1, x0=0, x1=8: [sel[y * 8 + x] for y in range(y0, y1) for x in range(x0, x1)]
    assert _union(rows(0, 2)) == (17, 8, 0, 8)
    for y in (2, 4, 6):
        assert _union(rows(y, y + 2)) == (14, 1, 0, 1)
    assert _union(rows(0, 1, 0, 4)) == (24, 1, 0, 1) and _union(rows(0, 1, 4, 8)) == (24, 0, 0, 0)
    assert _union(rows(1, 2, 0, 4)) == (17, 1, 0, 1) and _union(rows(1, 2, 4, 8)) == (17, 0, 0, 0)
    return case


LIST_SOLVES = 16    # every 4-cell item solved by the list pass; nothing left to k_oi


# ---- a generic structure function ---------------------------------------------------------------------------------------------------------
def cressman_h():
    """CressmanStructure(h) with h = the Barnes localization radius the tiles are built for: the same cells reach the same observations"""
    return float(np.float32(_radius()))


# ---- running a case on the GPU --------------------------------------------------------------------------------------------------------------
def run(case, mp=MP, structure=None, allow_extrapolation=True, variance=False, seed=0):
    """-> (analysis, variance or None, oi_last_stats())"""
    import gridpp_amd as gridpp
    grid, points = gridpp.Grid(case["lats"], case["lons"]), gridpp.Points(case["plat"], case["plon"])
    st = structure if structure is not None else gridpp.BarnesStructure(H)
    if variance:
        bvar = np.random.default_rng(seed).uniform(0.5, 2, case["bg"].shape).astype(np.float32)
        out, var = gridpp.optimal_interpolation_full(grid, case["bg"], bvar, points, case["obs"], case["ratios"], case["pbg"],
                                                     np.ones(case["plat"].size, np.float32), st, mp, allow_extrapolation)
        return np.asarray(out), np.asarray(var), gridpp.oi_last_stats()
    out = gridpp.optimal_interpolation(grid, case["bg"], points, case["obs"], case["ratios"], case["pbg"], st, mp, allow_extrapolation)
    return np.asarray(out), None, gridpp.oi_last_stats()


def record():
    """every array the golden file holds, by name, and the first-pass statistics asserted on the way: a declined tile would make the
    comparison with these bits vacuous"""
    import gridpp_amd as gridpp
    rec = {}

    def first_pass(s, name):
        assert s["union_kernel_ms"] > 0 and s["fallback_tiles"] == 0 and s["solves"] == 1, (name, s)
    for name in sorted(TILES):
        out, _, s = run(build(name))
        first_pass(s, name)
        rec[name] = out
    for name in WITH_VARIANCE:
        out, var, s = run(build(name), variance=True, seed=len(name))
        first_pass(s, name)
        rec[name + "_full"], rec[name + "_var"] = out, var
    out, _, s = run(one_cell())
    first_pass(s, "one_cell")
    rec["one_cell"] = out
    ext = []
    for c in extreme_cases():
        out, _, s = run(c, allow_extrapolation=False)
        first_pass(s, "extreme")
        ext.append(out)
    rec["extreme"] = np.stack(ext)
    for name, cases in (("dup", pivot_cases()), ("neg", negative_cases())):
        ends = [ending(c) for c in cases]
        rec[name + "_raised"], rec[name + "_out"] = np.array([e[0] for e in ends], np.float32), np.stack([e[1] for e in ends])
    assert rec["dup_raised"].any(), "no pair met a non-positive pivot"
    assert not rec["neg_raised"].any() and np.isfinite(rec["neg_out"]).all()     # (a Cholesky that went on past a negative pivot would return NaNs)
    out, _, s = run(list_case())
    assert s["fallback_tiles"] == 1 and s["fallback_subtiles"] == 0 and s["solves"] == LIST_SOLVES, s
    rec["list"] = out
    out, _, s = run(build("c19_e12"), structure=gridpp.CressmanStructure(cressman_h()))
    first_pass(s, "cressman")
    rec["cressman_c19_e12"] = out
    return rec
