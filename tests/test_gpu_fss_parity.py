"""GPU: gridpp_amd.fractions_skill_score against its numpy restatement (tests/fss_ref.py; tests/test_fss_api.py holds that to hand-worked
answers and to the composition users write today).

Tolerances, derived and not measured, with N = cells[h]: cells exact; fbs and fbs_worst within (N + 8) 2^-53 relative -- the
per-cell terms are the same IEEE operations on the same integers, only the order of the additions differs; fss within (2 N + 16) 2^-53
absolute, because fbs <= fbs_worst; NaN in the same places.  Every call is made twice and the two results compared bit for bit; every case
runs on the path the library picks and under the general-path override, the two compared with the same tolerance; every case runs from
numpy and once from torch device tensors, which must give the bits of the numpy call.

The path rule of gridpp_amd/csrc/fss.hip is restated here (path_of) and every case says which path it takes:
  march    hw <= FSS_FUSED_MAXHW, E <= 32767 and (2 hw + 1)^2 E < 2^bk, bk = (64 - 2 bn) / 2, bn the smallest width with (2 hw + 1)^2 < 2^bn
  general  everything else, and every call under GPP_FSS_GENERAL (= wide: 64-bit row sums as well)
and the planes of a cell are 8 bits wide up to E = 127, 16 up to 32767 and 32 beyond."""
import contextlib
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import fss_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
HWS = (0, 1, 2, 16, 17, 201)
OPS = (R.Lt, R.Leq, R.Gt, R.Geq)


@pytest.fixture(scope="module")
def gridpp():
    import gridpp_amd
    return gridpp_amd


@contextlib.contextmanager
def override(name, value):
    os.environ[name] = str(value)       # (conftest hands the GPP_* variables to gpp_set_path_override before every call, and clears them after)
    try:
        yield
    finally:
        del os.environ[name]


def lanes(hw):
    area, bn = (2 * hw + 1) ** 2, 1
    while area >= 1 << bn:
        bn += 1
    return (64 - 2 * bn) // 2, bn


def path_of(hw, E):
    from gridpp_amd import _capi
    return "march" if hw <= _capi.FSS_FUSED_MAXHW and E <= 32767 and (2 * hw + 1) ** 2 * E < 1 << lanes(hw)[0] else "general"


def same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def within(got, want, what):
    """got against the restatement (or another path) with the tolerances of the module docstring"""
    np.testing.assert_array_equal(got.cells, want.cells, err_msg=what)
    N = want.cells.astype(np.float64)[None, :]
    for name in ("fbs", "fbs_worst"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape and g.dtype == np.float64, (what, name)
        assert (np.abs(g - w) <= (N + 8) * 2.0 ** -53 * w).all(), (what, name, float(np.max(np.abs(g - w) / np.maximum(w, 1e-300))))
    assert (np.isnan(got.fss) == np.isnan(want.fss)).all(), what
    assert (np.isnan(got.fss) == (want.fbs_worst == 0)).all(), what
    on = ~np.isnan(want.fss)
    assert (np.abs(got.fss - want.fss)[on] <= np.broadcast_to((2 * N + 16) * 2.0 ** -53, want.fss.shape)[on]).all(), what


def run_case(gridpp, f, r, thr, hws=HWS, op=R.Gt, wide=False):
    """-> the restatement's result, after every comparison the module docstring lists"""
    import torch
    want = R.fss(f, r, thr, hws, op)
    got = gridpp.fractions_skill_score(f, r, thr, hws, op)
    assert isinstance(got, gridpp.FssResult) and got.cells.dtype == np.int64 and got.fss.shape == (len(thr), len(hws))
    within(got, want, "library path")
    assert same_bits(got, gridpp.fractions_skill_score(f, r, thr, hws, op)), "the second call differs"
    for value in ("1", "wide") if wide else ("1",):
        with override("GPP_FSS_GENERAL", value):
            general = gridpp.fractions_skill_score(f, r, thr, hws, op)
            again = gridpp.fractions_skill_score(f, r, thr, hws, op)
        within(general, want, "general path " + value)
        within(general, got, "general path " + value + " against the library's")
        assert same_bits(general, again), "the second general call differs"
    dev = gridpp.fractions_skill_score(torch.from_numpy(np.ascontiguousarray(f, F)).cuda(), torch.from_numpy(np.ascontiguousarray(r, F)).cuda(), thr, hws, op)
    assert all(isinstance(a, np.ndarray) for a in dev) and same_bits(dev, got), "device tensors differ from numpy"
    return want


def pair(rng, Y, X, bad=0.03, quantum=None):
    yy, xx = np.meshgrid(np.arange(Y), np.arange(X), indexing="ij")
    smooth = np.sin(yy / 9.0) + np.cos(xx / 13.0)
    f, r = (smooth + rng.normal(0, 0.5, (Y, X))).astype(F), (smooth + rng.normal(0, 0.5, (Y, X))).astype(F)
    if quantum:
        f, r = (np.round(f / quantum) * quantum).astype(F), (np.round(r / quantum) * quantum).astype(F)
    for a in (f, r):
        hit = rng.random((Y, X)) < bad
        a[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(hit.sum()))
    return f, r


# ---- shapes: one cell, one short of / equal to / one past the tile, more than one strip and chunk ---------------------------------------------
@pytest.mark.parametrize("Y", (1, 31, 32, 33, 67))
@pytest.mark.parametrize("X", (1, 63, 64, 65, 131))
def test_shapes(gridpp, Y, X):
    assert [path_of(h, 1) for h in HWS] == ["march"] * 4 + ["general"] * 2
    f, r = pair(np.random.default_rng(1000 * Y + X), Y, X)
    run_case(gridpp, f, r, [0.1, 0.9])


# ---- thresholds: below every value, above every value (NaN), equal to values present in both fields --------------------------------------------
@pytest.mark.parametrize("T", (1, 2, 5))
def test_thresholds(gridpp, T):
    f, r = pair(np.random.default_rng(7), 67, 131, quantum=0.25)
    assert (f == F(0.5)).any() and (r == F(0.5)).any()
    thr = {1: [0.5], 2: [-math.inf, 50.0], 5: [-50.0, 0.5, 50.0, math.inf, 0.25]}[T]
    want = run_case(gridpp, f, r, thr)
    for t, th in enumerate(thr):
        if th >= 50:
            assert np.isnan(want.fss[t]).all() and not want.fbs_worst[t].any()       # no event in either field
        if th <= -50:
            assert (want.fss[t] == 1).all() and not want.fbs[t].any()                # every counting cell is an event in both


def test_the_four_operators_at_a_tie(gridpp):
    f, r = pair(np.random.default_rng(8), 67, 131, quantum=0.25)
    res = {op: run_case(gridpp, f, r, [0.5], (0, 2, 17), op) for op in OPS}
    assert not np.array_equal(res[R.Gt].fbs, res[R.Geq].fbs) and not np.array_equal(res[R.Lt].fbs, res[R.Leq].fbs)
    for a, b in ((R.Gt, R.Leq), (R.Lt, R.Geq)):                                       # complements: Ff -> 1 - Ff and Fo -> 1 - Fo leave fbs alone
        np.testing.assert_allclose(res[a].fbs, res[b].fbs, rtol=1e-12)


# ---- invalid data -----------------------------------------------------------------------------------------------------------------------------
def test_fields_that_count_nowhere_and_in_one_cell(gridpp):
    f, r = pair(np.random.default_rng(9), 33, 65)
    none = np.full_like(r, np.nan)
    want = run_case(gridpp, f, none, [0.1])
    assert not want.cells.any() and np.isnan(want.fss).all()
    run_case(gridpp, np.full_like(f, np.inf), r, [0.1])
    one = none.copy()
    one[20, 40] = 1.0
    f[20, 40] = 2.0
    want = run_case(gridpp, f, one, [0.1, 1.5])
    reach = lambda h: (min(32, 20 + h) - max(0, 20 - h) + 1) * (min(64, 40 + h) - max(0, 40 - h) + 1)   # the cells whose window holds (20, 40)
    assert want.cells.tolist() == [reach(h) for h in HWS] == [1, 9, 25, 29 * 33, 30 * 35, 33 * 65]
    assert (want.fss[0] == 1).all() and (want.fss[1] == 0).all()


# ---- ensembles: every width of a plane's cell, members invalid at random, whole cells invalid -------------------------------------------------
def cube_of(rng, Y, X, E, all_valid=False):
    f, r = pair(rng, Y, X, bad=0.0 if all_valid else 0.03)
    cube = (f[:, :, None] + rng.normal(0, 0.4, (Y, X, E))).astype(F)
    if not all_valid:
        hit = rng.random(cube.shape) < 0.1
        cube[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(hit.sum()))
        cube[rng.random((Y, X)) < 0.05] = np.nan                                     # whole cells without a valid member
    return cube, r


@pytest.mark.parametrize("E", (1, 2, 50, 127, 128, 255, 256, 257))
def test_ensembles(gridpp, E):
    cube, r = cube_of(np.random.default_rng(E), 33, 65, E)
    m = np.isfinite(cube).sum(axis=2)
    if E > 1:
        assert m.min() == 0 and len(np.unique(m)) > 2                                # cells differ in m: the pooled definition is what is pinned
    assert [path_of(h, E) for h in HWS] == ["march"] * 4 + ["general"] * 2
    run_case(gridpp, cube, r, [-0.3, 0.4, 0.4, 1.1, 9.0], wide=E in (2, 257))


def test_wider_planes_and_thresholds_beyond_a_batch(gridpp):
    """E beyond 32767: 32-bit planes, no march at any half width; 11 thresholds: more than the eight the member pass carries in registers"""
    rng = np.random.default_rng(3)
    for E in (32767, 32768):
        cube, r = cube_of(rng, 3, 5, E)
        assert [path_of(h, E) for h in (0, 1, 2, 7)] == ["march" if E == 32767 else "general"] * 4
        run_case(gridpp, cube, r, [0.2], (0, 1, 2, 7))
    cube, r = cube_of(rng, 33, 65, 20)
    run_case(gridpp, cube, r, list(np.linspace(-1.5, 1.5, 11)), (1, 17))


@pytest.mark.parametrize("E", (2, 50))
def test_all_valid_cube_against_the_librarys_own_neighbourhood(gridpp, E):
    """every member valid: Ff is the neighbourhood Mean of the per-cell probabilities k / E, which the library's neighbourhood gives in float32"""
    cube, r = cube_of(np.random.default_rng(40 + E), 67, 131, E, all_valid=True)
    r[rng_block()] = np.nan
    thr = [0.0, 0.8]
    want = run_case(gridpp, cube, r, thr)
    counts = np.isfinite(r)
    for t, th in enumerate(thr):
        pf = np.where(counts, (cube > F(th)).sum(axis=2) / F(E), np.nan).astype(F)
        po = np.where(counts, (r > F(th)).astype(F), np.nan).astype(F)
        for j, h in enumerate(HWS):
            mf = np.asarray(gridpp.neighbourhood(pf, h, gridpp.Mean), np.float64)
            mo = np.asarray(gridpp.neighbourhood(po, h, gridpp.Mean), np.float64)
            on = ~np.isnan(mf)
            N = int(on.sum())
            assert N == want.cells[j]
            comp = R.value(float(((mf[on] - mo[on]) ** 2).sum()), float((mf[on] ** 2 + mo[on] ** 2).sum()))
            assert abs(comp - want.fss[t, j]) <= 2.0 ** -22 + (2 * N + 16) * 2.0 ** -53, (th, h)


def rng_block():
    return (slice(20, 45), slice(50, 90))


# ---- packing bounds -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", (260, 261))
@pytest.mark.parametrize("E", (1, 50))
def test_window_sums_past_16_bits(gridpp, E, side):
    """half width 130, every cell an event in both fields: on 260 x 260 every window is clipped and the largest is the field, 67 600 (n, O)
    and 67 600 E (K, M); on 261 x 261 the centre's window is whole, 68 121 and 68 121 E = 3 406 050 at E = 50.  Past any 16-bit lane; the
    general path"""
    assert path_of(130, E) == "general" and path_of(16, E) == "march"
    f = np.ones((side, side, E), F) if E > 1 else np.ones((side, side), F)
    r = np.ones((side, side), F)
    want = run_case(gridpp, f, r, [0.5], (16, 130), wide=True)
    assert want.cells.tolist() == [side * side] * 2 and not want.fbs.any() and (want.fbs_worst == 2 * side * side).all()
    k, m, o, c = R.cell_integers(f, r, 0.5)
    assert R.box_sum(k, 130).max() == side * side * E > 65535 and R.box_sum(c, 130).max() == side * side == (68121 if side == 261 else 67600)


@pytest.mark.parametrize("E,path", ((1925, "march"), (1926, "general")))
def test_the_last_ensemble_size_of_the_march_at_its_widest_window(gridpp, E, path):
    """hw = 16: bn = 11, bk = 21; 1089 * 1925 = 2 096 325 < 2^21 <= 1089 * 1926 -- with every member an event the K and M lanes are as full as they get"""
    assert lanes(16) == (21, 11) and path_of(16, E) == path and 1089 * 1925 < 1 << 21 <= 1089 * 1926
    cube, r = np.ones((35, 66, E), F), np.ones((35, 66), F)
    cube[3, 5, ::2] = 0.0
    r[30, 60] = 0.0
    run_case(gridpp, cube, r, [0.5], (16,))


# ---- a workgroup that marches through several chunks: the ring wraps ---------------------------------------------------------------------------
def march_launch(Y, X, fill=1024):
    """the launch rule of the fused path (gridpp_amd/csrc/fss.hip, FssCall::march) -> SH, the number of row segments"""
    from gridpp_amd import _capi
    W, CH = _capi.FSS_TILE_COLS, _capi.FSS_TILE_ROWS
    strips = -(-X // W)
    segs = max(1, min(-(-fill // strips), -(-Y // CH)))
    SH = -(-(-(-Y // segs)) // CH) * CH
    while -(-Y // SH) > 65535:
        SH += CH
    return SH, -(-Y // SH)


def march_chunks(Y, SH, hw):
    """chunks of CH rows that the workgroup of every segment loads (k_fss_march: nchunk)"""
    from gridpp_amd import _capi
    CH = _capi.FSS_TILE_ROWS
    return [(min(Y, ya + SH) - 1 + hw - (ya - hw)) // CH + 1 for ya in range(0, Y, SH)]


def test_march_through_many_chunks(gridpp):
    Y, X = 200, 70
    assert march_launch(Y, X) == (32, 7) and march_launch(Y, X, 1) == (224, 1) and march_launch(Y, X, 4) == (128, 2)
    assert [march_chunks(Y, 224, h) for h in (0, 1, 16)] == [[7], [7], [8]] and march_chunks(Y, 128, 16) == [5, 4]
    f, r = pair(np.random.default_rng(11), Y, X)
    cube, _ = cube_of(np.random.default_rng(12), Y, X, 5)
    for fcst in (f, cube):
        plain = gridpp.fractions_skill_score(fcst, r, [0.1, 0.9], (0, 1, 16))
        within(plain, R.fss(fcst, r, [0.1, 0.9], (0, 1, 16)), "segments of one chunk")
        for fill in (1, 4):
            with override("GPP_FSS_FILL", fill):                      # run_case nests the general-path override in it and runs device tensors
                run_case(gridpp, fcst, r, [0.1, 0.9], (0, 1, 16))
                got = gridpp.fractions_skill_score(fcst, r, [0.1, 0.9], (0, 1, 16))
            within(got, plain, "fill %d" % fill)


# ---- the hand-worked answers ----------------------------------------------------------------------------------------------------------------------
def test_hand_worked_answers(gridpp):
    f, r = np.zeros((3, 3), F), np.zeros((3, 3), F)
    f[0, 0] = r[2, 2] = 1
    run_case(gridpp, f, r, [0.5], (0, 1, 2))
    got = gridpp.fractions_skill_score(f, r, [0.5], (0, 1, 2))
    close = lambda g, w: abs(g - float(w)) <= 4 * math.ulp(float(w))
    assert got.cells.tolist() == [9, 9, 9]
    assert got.fbs[0, 0] == 2 and got.fbs_worst[0, 0] == 2 and got.fss[0, 0] == 0
    assert close(got.fbs[0, 1], Fraction(17, 72)) and close(got.fbs_worst[0, 1], Fraction(169, 648))
    assert abs(got.fss[0, 1] - 16 / 169) <= (2 * 9 + 16) * 2.0 ** -53
    assert got.fbs[0, 2] == 0 and close(got.fbs_worst[0, 2], Fraction(2, 9)) and got.fss[0, 2] == 1
