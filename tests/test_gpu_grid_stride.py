"""GPU: every grid-stride loop outside the OI and EnSI units beyond its first trip, at small shapes.

Most kernels launch `grid_capped(items, cap)` workgroups and stride over the rest; the caps are sized for the chip, so without help only a
field of millions of rows sends a workgroup through its loop twice.  The path override GPP_GRID_CAP=n caps every such grid at n workgroups as
well.  Every case here runs a call three times -- under the library's defaults, under GPP_GRID_CAP=1 (one workgroup makes every trip, in
order) and under a cap of 2 or 3 (the trips are dealt unevenly and the ragged last tile falls on another workgroup than 0; where the issue
fixes a shape for which one cap cannot do both -- five tiles, three row blocks -- the case runs under both 2 and 3) -- and compares
  * with the restatement, by exactly the comparison the kernel's parity test uses (bit for bit where that is bit for bit, crps_close with
    crps_slack for the CRPS, the derived bounds of the FSS), and
  * bit for bit with the default-grid call wherever one workgroup (or one thread) owns an output, or the per-workgroup partials are exact.
The data is laid out so that a trip differs from the one before it in the same workgroup: other pattern kinds and NaN counts per lane, an
all-NaN tile behind rows without a NaN, zeros of both signs next to rows with none, levels that take another branch per row, row blocks
whose scale differs by a factor of ten.

kernel                          launch site                    cap              2nd trip reached by       against the default grid
------------------------------  -----------------------------  ---------------  ------------------------  ------------------------------------
k_rank_tile                     rows_rank.hip calc_ranks       2^20 tiles       GPP_GRID_CAP              equal bits (a lane owns a row)
k_reorder_tile                  rows_rank.hip reorder          2^20 tiles       GPP_GRID_CAP              equal bits
k_crps_tile                     rows_rank.hip calc_crps        2^20 tiles       GPP_GRID_CAP              equal bits (two double sums per lane)
k_rank_block<0>, <1>            rows_rank.hip                  2^20 rows        GPP_GRID_CAP              equal bits (a workgroup owns a row)
k_sort_block                    rows_rank.hip                  2^20 rows        GPP_GRID_CAP              equal bits
k_crps_block                    rows_rank.hip calc_crps        2^20 rows        GPP_GRID_CAP              equal bits (fixed tree inside the row)
k_crps_long                     rows_rank.hip calc_crps        2^20 rows        GPP_GRID_CAP              equal bits
k_rowsq_tile                    rows_quantiles.hip             2^20 tiles       GPP_GRID_CAP              equal bits
k_rowsq_block                   rows_quantiles.hip             2^20 rows        GPP_GRID_CAP              equal bits
k_rows_tile                     rows_select.hip rows_quantile  256 waves_per_cu GPP_GRID_CAP, natural     equal bits
k_rows_block                    rows_select.hip rows_quantile  2048             GPP_GRID_CAP, natural     equal bits (integer histograms)
k_window_scan<1|4, false|true>  window.hip window_launch       2^22 row blocks  GPP_GRID_CAP              equal bits (a lane owns a row)
k_window_gather<1|4>            window.hip window_launch       2^22 row blocks  GPP_GRID_CAP              equal bits
k_window_from_planes            window.hip window_launch       2^22 workgroups  GPP_GRID_CAP (natural: test_gpu_window_large.py)  equal bits
k_window_gather_rows            window.hip window_launch       2^22 workgroups  GPP_GRID_CAP (natural: test_gpu_window_large.py)  equal bits
k_structure_corr_many           structure_corr.hip             2048             GPP_GRID_CAP, natural     equal bits (a lane owns a point)
k_member_pass<0|1|2>            neighbourhood.hip              256 waves_per_cu GPP_GRID_CAP              equal bits (a lane owns a cell)
k_qf_count<NL>                  neighbourhood.hip              256 waves_per_cu GPP_GRID_CAP              equal bits (byte counts per cell)
k_curve_shared                  curve.hip launch_shared        2 per CU         GPP_GRID_CAP, natural (test_gpu_curve_parity.py)  equal bits
k_fss_classify, k_fss_count     fss.hip FssCall::classify      2048             GPP_GRID_CAP              exact planes: equal bits on the march path
k_fss_rows                      fss.hip FssCall::general       2048             GPP_GRID_CAP              exact integer row sums
k_fss_cols                      fss.hip FssCall::general       2048 (= nblk)    GPP_GRID_CAP              NOT exact: one double partial of (K/M - O/n)^2
                                                                                                          terms per workgroup, so fbs and fbs_worst keep the
                                                                                                          parity test's bounds ((N + 8) 2^-53 relative, fss
                                                                                                          (2 N + 16) 2^-53) against the restatement and the
                                                                                                          default grid; cells (integers) equal
k_score_counts                  score.hip gpp_calc_score       8192             GPP_GRID_CAP, natural (test_gpu_score_parity.py)  exact 64-bit integer counts: equal bits
k_score_rows, k_score_cols      score.hip general path         own (SCORE_FILL) GPP_GRID_CAP, GPP_SCORE_FILL  equal bits (a thread owns a run)
k_mo_keys                       metric_optimizer.hip           8192             GPP_GRID_CAP, natural     equal bits (per element)
k_gamma_inv, k_gamma_transform  gamma.hip                      2048             GPP_GRID_CAP, natural (test_gpu_gamma_parity.py)   equal bits (per element)
k_pointwise<...>                pointwise.hip                  2048             GPP_GRID_CAP, natural (test_gpu_pointwise_parity.py) equal bits (per element)

tests/test_grid_stride_table.py reads this table: a kernel with a loop over gridDim.x that is missing here fails there.

Measured on the MI355X: the 36 test functions of this file take 3.9 s together; the slowest call is test_metric_optimizer with 0.33 s (then
test_structure_corr_many with 0.23 s), the one-off module setup (loading the library and torch) 1.4 s."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

from tests import fss_ref, gamma_ref, metric_optimizer_ref, pointwise_ref, rows_rank_ref, rows_select_ref, score_ref, structure_corr_cases, window_ref
from tests import test_gpu_fss_parity as FP
from tests import test_gpu_metric_optimizer_parity as MP
from tests import test_gpu_neighbourhood_edges as NE
from tests import test_gpu_quantiles_parity as QP
from tests import test_gpu_ranks_parity as RK
from tests import test_gpu_rows_select as RS
from tests import test_gpu_score_parity as SP
from tests import test_gpu_structure_corr_many as SC
from tests import test_gpu_window_parity as WP

pytestmark = pytest.mark.gpu
F = np.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def api():
    import torch
    import gridpp_amd as gridpp
    assert gridpp.device_count() > 0
    return gridpp, torch


@contextlib.contextmanager
def overrides(gridpp, **settings):
    """the overrides of `settings` (None: not set) for the block; none is set before it and none after it"""
    names = sorted(k for k, v in settings.items() if v is not None)
    assert gridpp.active_overrides() == []
    try:
        for k in names:
            gridpp.set_path_override(k, str(settings[k]))
        assert sorted(gridpp.active_overrides()) == names
        yield
    finally:
        for k in settings:
            gridpp.set_path_override(k, None)
        assert gridpp.active_overrides() == []


def bits_equal(got, base, what):
    """two results of the same call (arrays or tuples of arrays): the same bytes"""
    if isinstance(got, (tuple, list)):
        assert len(got) == len(base), what
        for k, (g, b) in enumerate(zip(got, base)):
            bits_equal(g, b, (what, k))
        return
    g, b = np.ascontiguousarray(got), np.ascontiguousarray(base)
    assert g.dtype == b.dtype and g.shape == b.shape, (what, g.dtype, b.dtype, g.shape, b.shape)
    if g.tobytes() != b.tobytes():
        gb, bb = (x.reshape(-1).view(np.uint8).reshape(x.size, x.itemsize) for x in (g, b))
        diff = np.flatnonzero((gb != bb).any(axis=1))[:8]
        raise AssertionError((what, "differs from the default grid at", diff, g.reshape(-1)[diff], b.reshape(-1)[diff]))


def on_every_grid(gridpp, caps, call, check, what, equal_bits=True, **paths):
    """call() under the default grid, then under every cap of `caps`; check(result) each time, and the default grid's bits where they hold"""
    with overrides(gridpp, **paths):
        base = call()
    check(base)
    for cap in caps:
        with overrides(gridpp, GPP_GRID_CAP=cap, **paths):
            got = call()
        check(got)
        if equal_bits:
            bits_equal(got, base, (what, "GPP_GRID_CAP", cap))
    return base


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


# ---- the override itself --------------------------------------------------------------------------------------------------------------------
def test_the_override_is_listed_and_values_below_one_do_nothing(api):
    gridpp, torch = api
    a = RK.device(RK.data(50, 129))
    base = host(gridpp.calc_ranks(a))
    for value in ("0", "-3", "x", "", "2x", "1", "2", "4294967297"):
        with overrides(gridpp, GPP_GRID_CAP=value):
            assert gridpp.active_overrides() == ["GPP_GRID_CAP"]          # listed whatever the value says: bench.py refuses to run with it
            bits_equal(host(gridpp.calc_ranks(a)), base, value)
    RK.same_ranks(base, rows_rank_ref.rows_of(rows_rank_ref.ranks, RK.data(50, 129)).astype(np.int32))


# ---- rows_rank --------------------------------------------------------------------------------------------------------------------------------
RANK_TILE_LENGTHS = (1, 7, 50, 160)      # 1: the len == 1 case of the magic division; 160: the largest LDS, the byte areas right behind the keys
RANK_TILE_ROWS = 4 * 64 + 1              # five tiles, the last one of one row


@functools.lru_cache(maxsize=None)
def rank_tile_want(L):
    """257 rows of the parity test's kinds, row n of kind (n + shift) % 12: lane l of consecutive tiles holds kinds that differ by 64 % 12 = 4.
    The even lanes of tiles 0 and 1 hold rows without a NaN and tile 2 is all NaN: whichever of them a workgroup has just left (tile 1 under a
    cap of 1, tile 0 under a cap of 2), a slot byte it left behind is a position where the all-NaN tile must write NaN.  The one row of tile 4
    is half NaN and follows a row without one under a cap of 3."""
    shift = 5 * RANK_TILE_LENGTHS.index(L)
    a, t = np.array(RK.data(L, RANK_TILE_ROWS, shift)), RK.data(L, RANK_TILE_ROWS, shift + 3)
    rng = np.random.default_rng(77 + L)
    a[0:128:2] = rng.normal(0, 1, (64, L)).astype(F)
    a[128:192] = np.nan
    a[256] = RK.pattern_row(9, L, rng, 0.5)
    a.setflags(write=False)
    return RK.Want(a, t)


@pytest.mark.parametrize("L", RANK_TILE_LENGTHS)
def test_rows_rank_tile(api, L):
    gridpp, torch = api
    w = rank_tile_want(L)
    nans = np.isnan(w.a).sum(axis=1)
    assert not nans[0:128:2].any() and (nans[128:192] == L).all()
    for k in range(3):                                                   # consecutive full tiles differ in the NaN counts of their lanes
        assert (nans[64 * k:64 * k + 64] != nans[64 * k + 64:64 * k + 128]).any(), k
    a, t, y = RK.device(w.a), RK.device(w.t), RK.device(w.y)
    results = []

    def call():
        ranks, srt, got = RK.check_all(gridpp, w, RANK_TILE_ROWS, a, t, y)   # the parity test's comparison of all four functions
        return host(ranks), host(srt), host(got), host(gridpp.calc_crps(a, y))

    on_every_grid(gridpp, (1, 2, 3), call, results.append, ("rows_rank tile", L), GPP_ROWS_RANKS="tile")
    assert len(results) == 4


RANK_BLOCK_LENGTHS = (161, 257, 1025)


@functools.lru_cache(maxsize=None)
def rank_block_want(L):
    """5 rows.  Zeros of both signs in rows 0, 3 and 4, none in rows 1 and 2: one workgroup (cap 1) goes both -> none -> none -> both -> both,
    two (cap 2) go 0 -> 2 -> 4 (both -> none -> both) and 1 -> 3 (none -> both): k_sort_block's rewrite of the run of zeros follows a row
    without it and the reverse in either deal."""
    rng = np.random.default_rng(500 + L)
    kinds = (10, 0, 9, 6, 10)
    a = np.stack([RK.pattern_row(p, L, rng, 0.1) for p in kinds])
    t = np.stack([RK.pattern_row(p, L, rng, 0.1) for p in (0, 10, 6, 11, 3)])
    both = [bool((np.signbit(r) & (r == 0)).any() and (~np.signbit(r) & (r == 0)).any()) for r in a]
    assert both == [True, False, False, True, True], both
    a.setflags(write=False), t.setflags(write=False)
    return RK.Want(a, t)


@pytest.mark.parametrize("L", RANK_BLOCK_LENGTHS)
def test_rows_rank_block(api, L):
    gridpp, torch = api
    from gridpp_amd import _capi
    lib = _capi.lib()
    w = rank_block_want(L)
    a, t, y = RK.device(w.a), RK.device(w.t), RK.device(w.y)
    p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731

    def call():
        ranks, srt, got = RK.check_all(gridpp, w, 5, a, t, y)
        out = [host(ranks), host(srt), host(got), host(gridpp.calc_crps(a, y))]
        for want_ranks, want_sorted in ((1, 0), (0, 1)):                 # the C-ABI forms: k_rank_block<0> without a sorted row, k_sort_block alone
            r = torch.full((5, L), -7, dtype=torch.int32, device="cuda")
            s = torch.full((5, L), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert lib.gpp_calc_ranks(p(a), 5, L, p(r) if want_ranks else None, p(s) if want_sorted else None, _capi.MEM_DEVICE) == _capi.GPP_OK
            if want_ranks:
                RK.same_ranks(host(r), w.ranks)
                assert bool((s == -7).all())
            else:
                RK.identical(host(s), w.sorted)
                assert bool((r == -7).all())
            out += [host(r), host(s)]
        return tuple(out)

    on_every_grid(gridpp, (1, 2), call, lambda r: None, ("rows_rank block", L))


def test_rows_rank_long_crps(api):
    """k_crps_long: the one kernel of the long path with a loop over rows, and the len == 0 call that goes straight to it"""
    gridpp, torch = api
    w = RK.want(50, 129)
    a, t, y = RK.device(w.a[:5]), RK.device(w.t[:5]), RK.device(w.y[:5])

    def call():
        RK.check_all(gridpp, w, 5, a, t, y)
        return host(gridpp.calc_crps(a, y))

    on_every_grid(gridpp, (1, 2), call, lambda r: None, "rows_rank long", GPP_ROWS_RANKS="long")
    empty, zeros = torch.empty((5, 0), device="cuda"), torch.zeros(5, device="cuda")

    def no_members():
        return host(gridpp.calc_crps(empty, zeros))

    def all_nan(r):
        assert r.shape == (5,) and np.isnan(r).all()

    on_every_grid(gridpp, (1, 2), no_members, all_nan, "rows_rank len 0")


# ---- rows_quantiles ---------------------------------------------------------------------------------------------------------------------------
QUANTILE_LEVELS = ("ends", "seventeen", "repeated")   # 0, 1 and NaN among interior levels; two chunks of staged results; unsorted and repeated


@pytest.mark.parametrize("L", (1, 50, 160))
def test_rows_quantiles_tile(api, L):
    """257 rows: row n is row n % 129 of the parity test's data, so lane l of consecutive tiles holds rows 64 apart in it"""
    gridpp, torch = api
    pick = np.arange(257) % 129
    t = QP.device(QP.tile_data(L)[pick])
    for name in QUANTILE_LEVELS:
        want = QP.want("tile", L, name)[pick]
        on_every_grid(gridpp, (1, 2, 3), lambda: host(gridpp.calc_quantiles(t, QP.LEVELS[name])), lambda r: QP.identical(r, want),
                      ("rows_quantiles tile", L, name), GPP_ROWS_QUANTILES="tile")


@pytest.mark.parametrize("L", (161, 1025))
def test_rows_quantiles_block(api, L):
    gridpp, torch = api
    t = QP.device(QP.block_data(L))
    for name in QUANTILE_LEVELS:
        want = QP.want("block", L, name)
        on_every_grid(gridpp, (1, 2), lambda: host(gridpp.calc_quantiles(t, QP.LEVELS[name])), lambda r: QP.identical(r, want),
                      ("rows_quantiles block", L, name), GPP_ROWS_QUANTILES="block")


# ---- rows_select ------------------------------------------------------------------------------------------------------------------------------
SELECT_LEVELS = np.array([0.0, 1.0, NAN, 0.5, 0.37], F)   # min / max through s64, NaN, the radix passes through hist and s[], the successor search


def select_call(gridpp, torch, a, q):
    R, L = a.shape
    t, dq = torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(q).reshape(R, 1)).cuda()
    return lambda: host(gridpp.calc_quantile(t.reshape(R, 1, L), dq)).reshape(R)


@pytest.mark.parametrize("L", (1, 7, 50, 160))
def test_rows_select_tile(api, L):
    gridpp, torch = api
    a = np.array(RS.data(L, RANK_TILE_ROWS))
    a[65] = np.nan                                                      # an all-NaN row between two ordinary ones
    a[128:192:3] = np.nan                                               # and a third of the lanes of tile 2
    q = SELECT_LEVELS[np.arange(RANK_TILE_ROWS) % 5]                    # 64 % 5 = 4: a lane's level changes from tile to tile
    want = rows_select_ref.rows_quantile(a, q)
    on_every_grid(gridpp, (1, 2, 3), select_call(gridpp, torch, a, q), lambda r: RS.identical(r, want), ("rows_select tile", L), GPP_ROWS_SELECT="tile")
    half = rows_select_ref.rows_quantile(a, 0.5)                        # a scalar level: the other form of rs_level
    t = torch.from_numpy(a).cuda()
    on_every_grid(gridpp, (2,), lambda: host(gridpp.calc_quantile(t, 0.5)), lambda r: RS.identical(r, half), ("rows_select tile scalar", L), GPP_ROWS_SELECT="tile")


@pytest.mark.parametrize("L", (7, 161, 1025))
def test_rows_select_block(api, L):
    """5 rows, the third all NaN; the five rotations of the levels, so that each workgroup of either deal takes every branch after every other"""
    gridpp, torch = api
    b = RS.base(L)
    a = np.ascontiguousarray(b[[0, 1, 2, b.shape[0] - 8, 4]])            # rows of the neighbourhood tests and the all-zeros adversarial one
    a[2] = np.nan
    for rot in range(5):
        q = SELECT_LEVELS[(np.arange(5) + rot) % 5]
        want = rows_select_ref.rows_quantile(a, q)
        on_every_grid(gridpp, (1, 2), select_call(gridpp, torch, a, q), lambda r: RS.identical(r, want), ("rows_select block", L, rot), GPP_ROWS_SELECT="block")


@pytest.mark.parametrize("L,rows", [(161, 2049 + 3), (160, 768 * 64 + 65)], ids=["k_rows_block_2052_rows", "k_rows_tile_49217_rows"])
def test_rows_select_natural_caps(api, L, rows):
    """no override: the product's own caps (2048 workgroups; 256 * 3 at len 160).  The rows repeat a block of 129, so the restatement of one
    block is the whole check; 129 and the five levels are coprime to 64 and to the caps, so a workgroup's second trip holds other rows"""
    gridpp, torch = api
    block = np.array(RS.data(L, 129))
    block[65] = np.nan
    qb = SELECT_LEVELS[np.arange(129) % 5]
    want = rows_select_ref.rows_quantile(block, qb)
    pick = np.arange(rows) % 129
    assert gridpp.active_overrides() == []
    got = select_call(gridpp, torch, block[pick], qb[pick])()
    RS.identical(got, want[pick])
    assert gridpp.active_overrides() == []


# ---- window -----------------------------------------------------------------------------------------------------------------------------------
WINDOW_Y = 2 * WP.ROWS + 3                                               # three row blocks, the last one of three rows
WINDOW_TS = (WP.COLS + 1, 2 * WP.COLS + 4)                               # the scalar and the 16-byte form, more than one chunk
WINDOW_STATS = (window_ref.Sum, window_ref.Mean, window_ref.Count, window_ref.Median, window_ref.Max)
WINDOW_LENGTHS = ((3, False), (WP.FUSED_CENTRED, False), (WP.FUSED_BEFORE, True), (WP.FUSED_BEFORE + 2, True))


@pytest.mark.parametrize("kind", ("sprinkled", "nan_at_0"))
@pytest.mark.parametrize("T", WINDOW_TS)
def test_window(api, T, kind):
    """The rows of block b are 10^b times those of the parity test's content: a prefix or a count that the ring kept from the row block
    before shows in the first `back` columns.  The fused lengths run again under GPP_WINDOW_GENERAL: k_window_scan<., false> and <., true>,
    k_window_from_planes, k_window_gather and k_window_gather_rows all stride."""
    gridpp, torch = api
    a = WP.content(kind, WINDOW_Y, T, seed=T)
    for b in range(3):
        a[b * WP.ROWS:(b + 1) * WP.ROWS] *= F(10.0 ** b)
    d = torch.from_numpy(a).cuda()
    assert d.data_ptr() % 16 == 0
    for length, before in WINDOW_LENGTHS:
        fused = WP.is_fused(T, length, before)
        assert fused == (length != WP.FUSED_BEFORE + 2)
        for statistic in WINDOW_STATS:
            want = window_ref.window(a, length, statistic, before, False, False)
            for general in ((None, "1") if fused else (None,)):
                on_every_grid(gridpp, (1, 2), lambda: host(gridpp.window(d, length, statistic, before, False, False)),
                              lambda r: window_ref.same_bits(r, want), ("window", T, kind, length, before, statistic, general), GPP_WINDOW_GENERAL=general)
    want = window_ref.window(a, 5, window_ref.Mean, False, True, True)   # both flags once
    on_every_grid(gridpp, (1, 2), lambda: host(gridpp.window(d, 5, window_ref.Mean, False, True, True)), lambda r: window_ref.same_bits(r, want), ("window flags", T, kind))


# ---- structure_corr_many ----------------------------------------------------------------------------------------------------------------------
def test_structure_corr_many(api):
    """both entry points (records at stride 7, a point-set handle at stride 1) against the scalar call pair by pair"""
    gridpp, torch = api
    case, structure, per_centre = SC._case(0)
    centre, (lats, lons, elevs, lafs), points, expected = per_centre[0]
    for n in (257, 1000):
        handle = gridpp.Points(lats[:n], lons[:n], elevs[:n], lafs[:n])
        for (variant, background), values in expected.items():
            p1 = SC._p1(centre, variant)
            fn = structure.corr_background if background else structure.corr

            def check(r):
                assert r.dtype == F and r.shape == (n,) and SC._same(r, values[:n]), (n, variant, background)

            on_every_grid(gridpp, (1, 3), lambda: np.asarray(fn(p1, points[:n])), check, ("corr list", n, variant, background))
            on_every_grid(gridpp, (1, 3), lambda: np.asarray(fn(p1, handle)), check, ("corr handle", n, variant, background))
            on_every_grid(gridpp, (3,), lambda: host(fn(p1, handle, device="cuda")), check, ("corr handle device", n, variant, background))


def test_structure_corr_natural_cap(api):
    """2048 * 256 + 5 points, no override: the last five belong to the second trip of workgroup 0.  The points repeat the pool of 1000."""
    gridpp, torch = api
    case, structure, per_centre = SC._case(0)
    centre, (lats, lons, elevs, lafs), points, expected = per_centre[0]
    n = 2048 * 256 + 5
    pick = np.arange(n) % structure_corr_cases.N
    handle = gridpp.Points(lats[pick], lons[pick], elevs[pick], lafs[pick])
    small = gridpp.Points(lats, lons, elevs, lafs)
    assert gridpp.active_overrides() == []
    for background in (0, 1):
        values = expected["full", background]
        p1 = SC._p1(centre, "full")
        fn = structure.corr_background if background else structure.corr
        got = np.asarray(fn(p1, handle))
        assert got.dtype == F and got.shape == (n,)
        assert SC._same(got[:300], values[:300]) and SC._same(got[-300:], values[pick[-300:]])     # the scalar call, pair by pair
        assert SC._same(got[:1000], np.asarray(fn(p1, small)))                                     # the n = 1000 call on the overlap
        assert SC._same(got, values[pick])


# ---- neighbourhood member passes and the shared curve: clamps that went through std::min before ----------------------------------------------------
def test_neighbourhood_member_kernels(api):
    """37 x 45 cells = 26 tiles of 64 and one of 1: k_member_pass<0> from LDS (E = 20) and from memory (E = 161), k_qf_count (E = 64, ranked byte
    counts in super-tiles of four), k_member_pass<2> (E = 3) and k_member_pass<1> (T = 17: the unfused form), with the parity tests' measures"""
    gridpp, torch = api
    from oracle import oracle as O
    Y, X = 37, 45
    for E in (20, 161):
        f = NE.members(40 + E, Y, X, E)
        for stat, exact in ((gridpp.Mean, False), (gridpp.Max, True), (gridpp.Median, True)):
            want = O.neighbourhood(f, 3, stat)
            on_every_grid(gridpp, (1, 3), lambda: gridpp.neighbourhood(f, 3, stat), lambda r: NE.close(r, want, exact=exact), ("member pass", E, stat))
    for E, T, hw in ((64, 16, 15), (3, 16, 15), (3, 17, 17)):
        rng = np.random.default_rng(E * 1000 + T * 10 + hw)
        f = np.round(rng.uniform(-1, T + 1, (Y, X, E))).astype(F)
        f[rng.random(f.shape) < 0.02] = np.nan
        f[3:5, 7:9, :] = np.nan
        thr = np.arange(T, dtype=F)
        qf = rng.random((Y, X)).astype(F)
        qf[0, :5], qf[1, :5], qf[2, :5] = 0.0, 1.0, np.nan
        want = O.neighbourhood_quantile_fast(f, qf, hw, thr)
        on_every_grid(gridpp, (1, 3), lambda: gridpp.neighbourhood_quantile_fast(f, qf, hw, thr), lambda r: NE.same(r, want), ("quantile_fast", E, T, hw))


def test_shared_curve(api):
    """k_curve_shared with the curve staged in LDS (10 entries) and read through the caches (5000): 1003 values, four workgroups of work"""
    gridpp, torch = api
    from tests import curve_ref
    for nc in (10, 5000):
        rng = np.random.default_rng(nc)
        r, f = curve_ref.random_curves(rng, (), nc, "sorted")
        x = curve_ref.random_inputs(rng, (1003,), f)
        want = curve_ref.apply_curve(x, r, f, curve_ref.OneToOne, curve_ref.MeanSlope)
        on_every_grid(gridpp, (1, 3), lambda: gridpp.apply_curve(x, r, f, curve_ref.OneToOne, curve_ref.MeanSlope),
                      lambda got: np.testing.assert_array_equal(got, want), ("apply_curve", nc))


# ---- fss, score, metric_optimizer, gamma, pointwise: the override reaches them ----------------------------------------------------------------------
def test_fss(api):
    """67 x 131 cells under GPP_FSS_GENERAL: k_fss_classify (35 workgroups of work), k_fss_rows and k_fss_cols (5) stride, and `parts` is sized
    for the smaller nblk.  A cube of 33 x 65 x 50 for k_fss_count.  fbs / fbs_worst: the parity test's bounds (see the table); cells: equal."""
    gridpp, torch = api
    thr = [0.1, 0.9]
    f, r = FP.pair(np.random.default_rng(67131), 67, 131)
    cube, rc = FP.cube_of(np.random.default_rng(50), 33, 65, 50)
    for fc, rf, th in ((f, r, thr), (cube, rc, [-0.3, 0.4, 1.1])):
        want = fss_ref.fss(fc, rf, th, FP.HWS, fss_ref.Gt)
        state = {}

        def check(got):
            FP.within(got, want, "against the restatement")
            if "base" in state:
                FP.within(got, state["base"], "against the default grid")
                np.testing.assert_array_equal(got.cells, state["base"].cells)
            state.setdefault("base", got)
            assert FP.same_bits(got, gridpp.fractions_skill_score(fc, rf, th, FP.HWS, fss_ref.Gt)), "the second call differs"

        with overrides(gridpp, GPP_FSS_GENERAL="1"):
            check(gridpp.fractions_skill_score(fc, rf, th, FP.HWS, fss_ref.Gt))
        for cap in (1, 2):
            with overrides(gridpp, GPP_FSS_GENERAL="1", GPP_GRID_CAP=cap):
                check(gridpp.fractions_skill_score(fc, rf, th, FP.HWS, fss_ref.Gt))
        # the library's own paths: the planes of k_fss_classify / k_fss_count are exact and the march does not stride, so the half widths it
        # takes give the bits of the default grid
        march = [h for h in FP.HWS if FP.path_of(h, 1 if fc.ndim == 2 else fc.shape[2]) == "march"]
        assert len(march) >= 3
        on_every_grid(gridpp, (1, 2), lambda: tuple(gridpp.fractions_skill_score(fc, rf, th, march, fss_ref.Gt)), lambda r_: None, "fss march")


def test_score(api):
    gridpp, torch = api
    ref, fcst = SP.vectors(100003, 7 + 100003, True)                     # k_score_counts: 391 workgroups of work, exact integer counts
    dref, dfcst = torch.from_numpy(ref).cuda(), torch.from_numpy(fcst).cuda()
    for metric in score_ref.METRICS:
        want = score_ref.calc_score_vec(ref, fcst, 0.4, 0.6, metric)
        on_every_grid(gridpp, (1, 2), lambda: np.float32(gridpp.calc_score(dref, dfcst, 0.4, 0.6, metric)), lambda r: score_ref.same_bits(r, want), ("calc_score", metric))
    Y, X = SP.YS[-1], SP.XS[-1]                                          # 67 x 131: the general path's k_score_rows and k_score_cols
    lats, lons, plat, plon, obs, fc = score_ref.case_inputs(Y, X, True, "sprinkled", seed=1000 * Y + X)
    grid, points, og, op = SP.handles(gridpp, lats, lons, plat, plon, True)
    ref_grid = score_ref.gridded(og, op, obs, fc.shape)
    for hw in (2, SP.MAXHW + 1):
        a, b, c, d = score_ref.hoods(og, op, fc, obs, hw, score_ref.THRESHOLD, ref_grid)
        for metric in (score_ref.Ets, score_ref.Bias):
            want = score_ref.calc_score_table(a, b, c, d, metric)
            on_every_grid(gridpp, (1, 2), lambda: gridpp.neighbourhood_score(grid, points, fc, obs, hw, metric, score_ref.THRESHOLD),
                          lambda r: score_ref.same_bits(r, want), ("neighbourhood_score", hw, metric), GPP_SCORE_GENERAL="1")


def test_metric_optimizer(api):
    gridpp, torch = api
    n = metric_optimizer_ref.SIZES[-1]                                   # 1025: five workgroups of k_mo_keys
    for halves in (False, True):
        ref, fcst = MP.data(n, halves)
        for metric in metric_optimizer_ref.METRICS:
            want = np.array([MP.expected(n, halves, t, metric) for t in metric_optimizer_ref.THRESHOLDS], F)
            on_every_grid(gridpp, (1, 2), lambda: np.array([gridpp.get_optimal_threshold(ref, fcst, t, metric) for t in metric_optimizer_ref.THRESHOLDS], F),
                          lambda r: metric_optimizer_ref.same_bits(r, want), ("get_optimal_threshold", halves, metric))


def test_gamma(api):
    gridpp, torch = api
    from gridpp_amd import _capi
    g = gamma_ref.golden()
    n = 2 * _capi.GAMMA_BLOCK + 1                                        # three workgroups of work
    level, shape, scale, want = (gamma_ref.tile(x, n) for x in (g.gi_level, g.gi_shape, g.gi_scale, g.gi_want))

    def matches(expect, alternatives, *inputs):
        def check(r):
            idx = gamma_ref.mismatches(r, expect, alternatives)
            assert len(idx) == 0, gamma_ref.report(idx, r, expect, *inputs)
        return check

    on_every_grid(gridpp, (1, 2), lambda: gridpp.gamma_inv(level, shape, scale), matches(want, (), level, shape, scale), "gamma_inv")
    params, values, wanted, neighbours = next(iter(g.forward_sets()))
    v, wf, alt = gamma_ref.tile(values, n), gamma_ref.tile(wanted, n), [gamma_ref.tile(x, n) for x in neighbours]
    forward = gridpp.Gamma(*params).forward
    on_every_grid(gridpp, (1, 2), lambda: forward(v), matches(wf, alt, v), "Gamma.forward")
    params, values, wanted = next(iter(g.backward_sets()))
    v2, wb = gamma_ref.tile(values, n), gamma_ref.tile(wanted, n)
    backward = gridpp.Gamma(*params).backward
    on_every_grid(gridpp, (1, 2), lambda: backward(v2), matches(wb, (), v2), "Gamma.backward")


def test_pointwise(api):
    gridpp, torch = api
    from gridpp_amd import _capi
    n = 3 * _capi.POINTWISE_BLOCK * 4 + 5                                # three workgroups of four values per lane, and the tail launch
    for name in ("wind_speed", "wetbulb", "qnh"):
        args = pointwise_ref.seeded_inputs(name, n, offenders=False)
        want = getattr(pointwise_ref, name)(*args)
        dev = [torch.tensor(x, device="cuda") for x in args]

        def check(r):
            bad = pointwise_ref.mismatches(r, want, 0 if name in pointwise_ref.EXACT else pointwise_ref.RTOL)
            assert bad.size == 0, (name, bad[:5], r[bad[:5]], want[bad[:5]])

        on_every_grid(gridpp, (1, 2), lambda: host(getattr(gridpp, name)(*dev)), check, name)
    for tid, cls, params in pointwise_ref.transforms()[1:3]:
        for direction in ("forward", "backward"):
            values = pointwise_ref.seeded_values(direction, n)
            want = getattr(getattr(pointwise_ref, cls)(*params), direction)(values)
            fn = getattr(getattr(gridpp, cls)(*params), direction)
            d = torch.tensor(values, device="cuda")

            def check_t(r):
                bad = pointwise_ref.transform_mismatches(tid, direction, values, r, want)
                assert bad.size == 0, (tid, direction, bad[:5])

            on_every_grid(gridpp, (1, 2), lambda: host(fn(d)), check_t, (tid, direction))
