"""GPU: the branches of the score, curve, ensemble-downscaling and distance kernels that only a field of millions of cells makes the
launch rule choose, reached on small inputs through a path override each (or, for the curve kernel, by a length past one pass of its
capped launch), and compared bit for bit (NaNs in the same places) with the restatements the parity tests use and with the same call
under the library's defaults:

    k_score_march        GPP_SCORE_FILL: one row segment per strip, so that a workgroup marches through three to seven chunks with the
                         ring of row counts wrapping, and segments of two chunks with a run-in and a ragged last one; one field of
                         2.1 M cells where the library picks such segments on its own
    k_curve_shared       lengths beyond P = 2 * compute units * 1024 * 4 values (P / 4 in the scalar form): further grid-stride trips
    k_ens_mask_rows /    GPP_ENSEMBLE_SLAB: ten slabs with a ragged last one, one cell per slab, a single slab; q0 > 0 and the scratch
    k_ens_rows_result    reused from slab to slab
    k_knn_max_distance   GPP_KNN_SLAB: slabs of seven locations (ragged last one), of one location, a single slab; queries and output
                         offset by q0 while the scratch starts again at 0

The only tolerance is the one tests/test_gpu_radius_parity.py states and justifies for the great-circle distance against the oracle
(rtol 1e-5, atol 5 cm: double trigonometry of two libms); against the call with no override that case is bit-equal too."""
import contextlib
import functools

import numpy as np
import pytest

from tests import curve_ref as CR
from tests import ensemble_downscaling_ref as ER
from tests import score_ref as R

pytestmark = pytest.mark.gpu

from gridpp_amd import _capi   # noqa: E402

F = np.float32
W, CH, MAXHW = _capi.SCORE_TILE_COLS, _capi.SCORE_TILE_ROWS, _capi.SCORE_FUSED_MAXHW
ROW_CAP = _capi.ENSEMBLE_ROW_CAP


@pytest.fixture(scope="module")
def gridpp():
    import gridpp_amd
    if gridpp_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return gridpp_amd


@contextlib.contextmanager
def override(gridpp, name, value):
    gridpp.set_path_override(name, str(value))
    try:
        assert name in gridpp.active_overrides()
        yield
    finally:
        gridpp.set_path_override(name, None)


# ---- score: GPP_SCORE_FILL --------------------------------------------------------------------------------------------------------
SCORE_HWS = (1, 2, MAXHW)
SCORE_OBS = ("several", "sprinkled")
# (Y, X, geodetic, fill) -> what the case claims: SH, the segments, and per half width the chunks every segment's workgroup runs
SCORE_CASES = [
    (2 * CH + 3, W + 1, False, 1, 3 * CH, 1, {1: [3], 2: [3], MAXHW: [4]}),
    (4 * CH, W, True, 1, 4 * CH, 1, {1: [5], 2: [5], MAXHW: [5]}),
    (5 * CH + 1, 2 * W + 3, False, 1, 6 * CH, 1, {1: [6], 2: [6], MAXHW: [7]}),
    # three strips x three segments of two chunks: rows 64 and 128 start a segment inside the field, the last one has 33 rows
    (5 * CH + 1, 2 * W + 3, False, 9, 2 * CH, 3, {1: [3, 3, 2], 2: [3, 3, 2], MAXHW: [3, 3, 3]}),
]


def score_launch(Y, X, fill=1024):
    """the launch rule of gpp_neighbourhood_score's fused path (gridpp_amd/csrc/score.hip) -> SH, the number of row segments"""
    strips = -(-X // W)
    segs = max(1, min(-(-fill // strips), -(-Y // CH)))
    SH = -(-(-(-Y // segs)) // CH) * CH
    while -(-Y // SH) > 65535:
        SH += CH
    return SH, -(-Y // SH)


def score_chunks(Y, SH, hw):
    """chunks of CH rows that the workgroup of every segment loads: its rows and hw more on either side (k_score_march: nchunk)"""
    out = []
    for ya in range(0, Y, SH):
        yb = min(Y, ya + SH)
        out.append((yb - 1 + hw - (ya - hw)) // CH + 1)
    return out


@functools.lru_cache(maxsize=None)
def score_inputs(Y, X, geodetic, obs):
    """the inputs of a parity case and its gridded reference (the oracle's linear scan: once per grid, shared by its fills, left unchanged)"""
    from oracle import oracle as O
    lats, lons, plat, plon, ref, fcst = R.case_inputs(Y, X, geodetic, obs, seed=1000 * Y + X)
    otype = O.Geodetic if geodetic else O.Cartesian
    ref_grid = R.gridded(O.Pts(lats.ravel(), lons.ravel(), ctype=otype), O.Pts(plat, plon, ctype=otype), ref, fcst.shape)
    return lats, lons, plat, plon, ref, fcst, ref_grid


def score_handles(gridpp, lats, lons, plat, plon, geodetic):
    from oracle import oracle as O
    ctype, otype = (gridpp.Geodetic, O.Geodetic) if geodetic else (gridpp.Cartesian, O.Cartesian)
    zy, zp = np.zeros_like(lats), np.zeros_like(plat)
    grid = gridpp.Grid(lats, lons, zy, zy, ctype)
    points = gridpp.Points(plat, plon, zp, zp, ctype)
    return grid, points, O.Pts(lats.ravel(), lons.ravel(), ctype=otype), O.Pts(plat, plon, ctype=otype)


@pytest.mark.parametrize("Y,X,geodetic,fill,SH,segments,chunks", SCORE_CASES, ids=["%dx%d-fill%d" % (c[0], c[1], c[3]) for c in SCORE_CASES])
def test_score_march_through_many_chunks(gridpp, Y, X, geodetic, fill, SH, segments, chunks):
    assert score_launch(Y, X, fill) == (SH, segments)
    assert score_launch(Y, X) == (CH, -(-Y // CH))          # no override: segments of one chunk, the two-chunk march of the parity tests
    for hw in SCORE_HWS:
        got = score_chunks(Y, SH, hw)
        print("score %d x %d fill %d hw %d: SH %d, %d segments, chunks per workgroup %s" % (Y, X, fill, hw, SH, segments, got))
        assert got == chunks[hw]
        if segments == 1:
            assert got[0] >= 3                              # the ring slot (k * CH + r) & 63 wraps from the third chunk on
        else:
            assert SH == 2 * CH and Y % SH != 0 and max(got) >= 3   # a ragged last segment
    for obs in SCORE_OBS:
        lats, lons, plat, plon, ref, fcst, ref_grid = score_inputs(Y, X, geodetic, obs)
        grid, points, og, op = score_handles(gridpp, lats, lons, plat, plon, geodetic)
        for hw in SCORE_HWS:
            a, b, c, d = R.hoods(og, op, fcst, ref, hw, R.THRESHOLD, ref_grid)
            for metric in R.METRICS:
                want = R.calc_score_table(a, b, c, d, metric)
                with override(gridpp, "GPP_SCORE_FILL", fill):
                    got = gridpp.neighbourhood_score(grid, points, fcst, ref, hw, metric, R.THRESHOLD)
                plain = gridpp.neighbourhood_score(grid, points, fcst, ref, hw, metric, R.THRESHOLD)
                with override(gridpp, "GPP_SCORE_GENERAL", 1):
                    general = gridpp.neighbourhood_score(grid, points, fcst, ref, hw, metric, R.THRESHOLD)
                assert got.dtype == np.float32 and got.shape == (Y, X)
                R.same_bits(got, want)
                R.same_bits(got, plain)
                R.same_bits(got, general)
    assert gridpp.active_overrides() == []


def test_score_march_on_a_field_where_the_library_picks_long_segments(gridpp):
    """1025 x 2048 cells: 32 strips, so the rule asks for 32 segments and gets SH = 2 CH (17 segments, the last one of one row) without
    any override.  One observation per cell, 180 m from its node on the 1 km grid, so that the gridded reference is the observation
    vector itself and the oracle's linear scan over 2.1 M x 2.1 M pairs is not needed."""
    Y, X = 32 * CH + 1, 32 * W
    assert score_launch(Y, X) == (2 * CH, 17)
    for hw in (1, MAXHW):
        got = score_chunks(Y, 2 * CH, hw)
        print("score %d x %d no override hw %d: SH %d, %d segments, chunks per workgroup %s" % (Y, X, hw, 2 * CH, len(got), got))
        assert got[:16] == [3] * 16 and got[16] == (1 if hw == 1 else 2)
    rng = np.random.default_rng(2048)
    lats, lons = R.geometry(Y, X, False)
    plat, plon = (lats + F(100)).ravel(), (lons - F(150)).ravel()
    ref = rng.random(Y * X).astype(F)
    fcst = rng.random((Y, X)).astype(F)
    fcst[rng.random((Y, X)) < 0.1] = np.nan
    grid, points, og, op = score_handles(gridpp, lats, lons, plat, plon, False)
    ref_grid = ref.reshape(Y, X)
    cats = [int(p.sum()) for p in R.planes(ref_grid, fcst, R.THRESHOLD)]
    assert min(cats) > Y * X // 8 and sum(cats) < Y * X                    # all four categories, and cells that count nowhere
    for hw in (1, MAXHW):
        a, b, c, d = R.hoods(og, op, fcst, ref, hw, R.THRESHOLD, ref_grid)
        for metric in R.METRICS:
            want = R.calc_score_table(a, b, c, d, metric)
            got = gridpp.neighbourhood_score(grid, points, fcst, ref, hw, metric, R.THRESHOLD)
            with override(gridpp, "GPP_SCORE_GENERAL", 1):
                general = gridpp.neighbourhood_score(grid, points, fcst, ref, hw, metric, R.THRESHOLD)
            R.same_bits(got, want)
            R.same_bits(general, got)
    assert gridpp.active_overrides() == []


# ---- curve: the grid stride of k_curve_shared -----------------------------------------------------------------------------------------
CURVES = [(10, "sorted"), (10, "nans"), (4097, "sorted"), (4097, "unsorted")]   # LDS + bisection, LDS + scans, caches + bisection, caches + scans
CURVE_BASE = 2003               # odd: tiled over the field, every base value meets every lane position and every slot of a 16-byte load
LONGEST_EXISTING = 1048579      # tests/test_gpu_curve_parity.py: (1 << 20) + 3 values


def curve_pass():
    """values one pass of k_curve_shared's capped launch covers in the 16-byte form: 2 workgroups per CU x 1024 lanes x 4 values"""
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count * 1024 * 4


def curve_base(nc, kind):
    rng = np.random.default_rng(nc + len(kind))
    r, f = CR.random_curves(rng, (), nc, kind)
    return r, f, CR.random_inputs(rng, (CURVE_BASE,), f)


@pytest.mark.parametrize("nc,kind", CURVES)
def test_curve_base_values_lie_below_inside_and_above_the_curve(nc, kind):
    r, f, base = curve_base(nc, kind)
    lo, hi = f[np.isfinite(f)].min(), f[np.isfinite(f)].max()
    ok = np.isfinite(base)
    assert (base[ok] < lo).any() and (base[ok] > hi).any() and ((base[ok] > lo) & (base[ok] < hi)).any()
    assert np.isnan(base).any() and np.isposinf(base).any() and np.isneginf(base).any()
    assert np.isin(base[ok], f).any()                       # and some lie on an entry
    assert CURVE_BASE % 2 == 1 and CURVE_BASE % 1024 != 0


def device_values(base, n, misaligned):
    """np.resize(base, n) in HBM: a tensor of its own (16-byte aligned), or a view 4 bytes behind such a boundary"""
    import torch
    if not misaligned:
        x = torch.from_numpy(np.resize(base, n)).cuda()
        assert x.data_ptr() % 16 == 0
        return x
    flat = torch.from_numpy(np.concatenate([np.zeros(1, F), np.resize(base, n)])).cuda()
    assert flat.data_ptr() % 16 == 0 and flat[1:].data_ptr() % 16 == 4
    return flat[1:]


@pytest.mark.parametrize("nc,kind", CURVES)
def test_curve_shared_takes_further_grid_stride_trips(gridpp, nc, kind):
    """Aligned: 16-byte form, P + 5 values (a second trip of one lane and a scalar tail) and 2 P + 4 * 1024 + 3 (two full trips and one
    workgroup of a third).  A view 4 bytes off: scalar form, one value per lane, P / 4 + 5 and P / 2 + 1027 values.  The restatement
    loops over the curve's entries in python, so it sees the 2003 base values once and both sides are tiled from there."""
    import torch
    P = curve_pass()
    assert P > LONGEST_EXISTING and P % 4096 == 0
    r, f, base = curve_base(nc, kind)
    want = CR.apply_curve(base, r, f, CR.MeanSlope, CR.NearestSlope)
    want_i = CR.interpolate(base, f, r)
    interp = (nc, kind) in ((10, "nans"), (4097, "sorted"))               # one staged curve with scans, one cached curve with bisection
    for n, misaligned, with_interpolate in ((P + 5, False, interp), (2 * P + 4 * 1024 + 3, False, False), (P // 4 + 5, True, interp),
                                            (P // 2 + 1027, True, False)):
        x = device_values(base, n, misaligned)
        got = gridpp.apply_curve(x, r, f, CR.MeanSlope, CR.NearestSlope)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (n,)
        np.testing.assert_array_equal(got.cpu().numpy(), np.resize(want, n), err_msg="nc %d %s n %d" % (nc, kind, n))
        if with_interpolate:
            np.testing.assert_array_equal(gridpp.interpolate(x, f, r).cpu().numpy(), np.resize(want_i, n), err_msg="interpolate n %d" % n)
    assert gridpp.active_overrides() == []


# ---- ensemble downscaling: GPP_ENSEMBLE_SLAB ------------------------------------------------------------------------------------------
LEVELS = np.array([-1.5, -0.5, 0.0, 0.5, 1.0, 2.5], F)   # few levels: member == threshold is common
ENS_OPS = (ER.Lt, ER.Leq, ER.Gt, ER.Geq)
ENS_STATS = [(s, None) for s in (ER.Mean, ER.Min, ER.Median, ER.Max, ER.Std, ER.Variance, ER.Sum, ER.Count)] + [(ER.Quantile, q) for q in (0.0, 0.3, 1.0)]
ENS_NE = ROW_CAP + 1
ENS_CELLS = 9 * 11
# members per slab -> the slabs the loop makes of the 99 cells
ENS_SLABS = [(10 * ENS_NE, [10] * 9 + [9]), (ENS_NE - 1, [1] * 99), (99 * ENS_NE, [99])]


class EnsembleCase:
    """5 x 7 input cells of ROW_CAP + 1 members, 9 x 11 output cells; cubes and per-cell thresholds filled as the `beyond` case of
    tests/test_gpu_ensemble_downscaling_parity.py fills them"""

    def __init__(self, gridpp, seed):
        from oracle import oracle as O
        rng = np.random.default_rng(seed)
        Y, X, E = 5, 7, ENS_NE
        ilats, ilons = np.meshgrid(np.linspace(50.0, 52.0, Y), np.linspace(5.0, 8.0, X), indexing="ij")
        olats, olons = np.meshgrid(np.linspace(49.9, 52.1, 9), np.linspace(4.9, 8.1, 11), indexing="ij")
        self.igrid, self.ogrid = gridpp.Grid(ilats, ilons), gridpp.Grid(olats, olons)
        self.idx = O.nearest_indices(O.Pts(ilats.ravel(), ilons.ravel()), O.Pts(olats.ravel(), olons.ravel()))
        self.oshape = olats.shape

        def cube():
            a = LEVELS[rng.integers(0, LEVELS.size, (Y, X, E))]
            a[rng.random(a.shape) < 0.08] = np.nan
            a[rng.random(a.shape) < 0.03] = np.inf
            a[rng.random(a.shape) < 0.03] = -np.inf
            a[rng.random((Y, X)) < 0.15] = np.nan   # cells with no valid member
            return a
        self.vt, self.vf, self.tv = cube() * F(3) + F(0.1), cube() - F(7), cube()
        thr = LEVELS[rng.integers(0, LEVELS.size, self.oshape)]
        flat = thr.reshape(-1)
        n = flat.size
        flat[rng.choice(n, max(1, n // 12), replace=False)] = np.nan
        flat[rng.choice(n, max(1, n // 20), replace=False)] = np.inf
        flat[rng.choice(n, max(1, n // 20), replace=False)] = -np.inf
        self.thr = thr

    def call(self, gridpp, op, stat, q):
        if stat == ER.Quantile:
            return gridpp.mask_threshold_downscale_quantile(self.igrid, self.ogrid, self.vt, self.vf, self.tv, self.thr, op, q)
        return gridpp.mask_threshold_downscale_consensus(self.igrid, self.ogrid, self.vt, self.vf, self.tv, self.thr, op, stat)


def ens_slabs(members, ne, nq):
    """the slab loop of gpp_mask_threshold_downscale (gridpp_amd/csrc/ensemble_downscale.hip) -> cells per slab"""
    slab = max(1, min(nq, members // ne))
    return [min(slab, nq - q0) for q0 in range(0, nq, slab)]


@pytest.fixture(scope="module")
def ensemble_case(gridpp):
    return EnsembleCase(gridpp, 12)


@pytest.fixture(scope="module")
def ensemble_expected(gridpp, ensemble_case):
    """(op, statistic, quantile) -> (the restatement, the call with no override), computed once and left unchanged"""
    from oracle import oracle as O
    c, out = ensemble_case, {}
    assert gridpp.active_overrides() == []
    for i, (stat, q) in enumerate(ENS_STATS):
        for shift in range(len(ENS_SLABS)):
            op = ENS_OPS[(i + shift) % 4]
            if (op, stat, q) not in out:
                out[op, stat, q] = (ER.mask(O, c.idx, c.vt, c.vf, c.tv, c.thr, op, stat, q), c.call(gridpp, op, stat, q))
    return out


@pytest.mark.parametrize("members,cells", ENS_SLABS, ids=["ten-slabs", "one-cell-slabs", "one-slab"])
def test_ensemble_rows_in_slabs(gridpp, ensemble_case, ensemble_expected, members, cells):
    c = ensemble_case
    assert ENS_NE > ROW_CAP and c.idx.size == ENS_CELLS
    assert ens_slabs(members, ENS_NE, ENS_CELLS) == cells
    assert ens_slabs(1 << 26, ENS_NE, ENS_CELLS) == [99]    # no override: one slab, as in every other test of this path
    shift = [m for m, _ in ENS_SLABS].index(members)
    used = set()
    for i, (stat, q) in enumerate(ENS_STATS):
        op = ENS_OPS[(i + shift) % 4]
        used.add(op)
        want, plain = ensemble_expected[op, stat, q]
        with override(gridpp, "GPP_ENSEMBLE_SLAB", members):
            got = c.call(gridpp, op, stat, q)
        assert got.dtype == F and got.shape == c.oshape
        np.testing.assert_array_equal(got, want, err_msg="op %d statistic %d quantile %r" % (op, stat, q))
        np.testing.assert_array_equal(got, plain, err_msg="op %d statistic %d quantile %r" % (op, stat, q))
    assert used == set(ENS_OPS)
    want = ensemble_expected[ENS_OPS[shift], ER.Mean, None][0].ravel()
    assert np.isnan(want).any() and np.isfinite(want[:10]).any() and np.isfinite(want[-9:]).any()   # (the first and the last slab are not all missing)
    assert gridpp.active_overrides() == []


@pytest.mark.parametrize("members,cells", ENS_SLABS, ids=["ten-slabs", "one-cell-slabs", "one-slab"])
def test_ensemble_random_choice_in_slabs(gridpp, ensemble_case, members, cells):
    c = ensemble_case
    for op in ENS_OPS:
        with override(gridpp, "GPP_ENSEMBLE_SLAB", members):
            got = gridpp.mask_threshold_downscale_consensus(c.igrid, c.ogrid, c.vt, c.vf, c.tv, c.thr, op, gridpp.RandomChoice).ravel()
        rows = ER.masked_rows(c.idx, c.vt, c.vf, c.tv, c.thr, op)
        some = np.isfinite(rows).any(axis=1)
        np.testing.assert_array_equal(np.isnan(got), ~some)
        assert some.any() and (~some).any()
        for k in np.nonzero(some)[0]:
            assert got[k] in rows[k][np.isfinite(rows[k])], (k, got[k])
    assert gridpp.active_overrides() == []


# ---- distance: GPP_KNN_SLAB ---------------------------------------------------------------------------------------------------------
KNN_NUMS = (1, 10, 200, 3000)
N_FROM, N_TO = 2500, 400
N_FEW = 250          # the points that num = 3000 searches (see test_distance_in_slabs)


def knn_slabs(entries, k, nq):
    """the slab loop of gpp_distance (gridpp_amd/csrc/radius.hip) -> locations per slab"""
    slab = max(1, min(nq, entries // k))
    return [min(slab, nq - q0) for q0 in range(0, nq, slab)]


@pytest.mark.parametrize("geodetic", [True, False], ids=["geodetic", "cartesian"])
def test_distance_in_slabs(gridpp, geodetic):
    """The point sets of test_distance_matches_oracle.  A location's candidate list is kept sorted by one thread in HBM, and a slab
    of one location is a launch of one thread: with all 2500 points in every list (num = 3000) the 900 such launches took two minutes.
    The slab loop depends on the number of locations and on the entries per slab, not on the size of `from`, so num = 3000 searches the
    first N_FEW of the 2500 points (still more asked for than there are, k = N_FEW); the other values of num search all of them."""
    import time
    from oracle import oracle as O
    from tests.test_gpu_radius_parity import _sets
    ct = 0 if geodetic else 1
    ilat, ilon, olat, olon = _sets(N_FROM, N_TO, geodetic, 77)
    op, oo = gridpp.Points(olat, olon, type=ct), O.Pts(olat, olon, ctype=ct)
    sources = {n: (gridpp.Points(ilat[:n], ilon[:n], type=ct), O.Pts(ilat[:n], ilon[:n], ctype=ct)) for n in (N_FROM, N_FEW)}
    lats, lons = np.meshgrid(np.linspace(olat.min(), olat.max(), 20), np.linspace(olon.min(), olon.max(), 25), indexing="ij")
    ogrid, oog = gridpp.Grid(lats, lons, type=ct), O.Pts(lats.ravel(), lons.ravel(), ctype=ct)
    for num in KNN_NUMS:
        n = N_FEW if num > N_FROM else N_FROM
        ip, oi_ = sources[n]
        k = min(num, n)
        assert (k == num) == (num <= N_FROM) and 20 <= N_FEW < KNN_NUMS[-1]
        assert knn_slabs(1 << 28, k, N_TO) == [N_TO] and knn_slabs(1 << 28, k, 500) == [500]   # no override: one slab
        for target, otarget, query_first, nq, shape in ((op, oo, True, N_TO, (N_TO,)), (ogrid, oog, False, 500, (20, 25))):
            t0 = time.perf_counter()
            plain = gridpp.distance(ip, target, num)
            ref = O.distance(oi_, otarget, num, query_first).reshape(shape)
            assert plain.shape == shape and (plain > 0).any()
            assert nq % 7 != 0
            # ragged last slab / one location per slab (k = 1: 0 entries is no positive value, the override does not count) / 400 locations
            for entries, slabs in ((7 * k, [7] * (nq // 7) + [nq % 7]), (k - 1, [1] * nq if k > 1 else [nq]), (400 * k, [400, 100][:-(-nq // 400)])):
                assert knn_slabs(entries if entries > 0 else 1 << 28, k, nq) == slabs
                with override(gridpp, "GPP_KNN_SLAB", entries):
                    got = gridpp.distance(ip, target, num)
                assert got.dtype == F and got.shape == shape
                np.testing.assert_array_equal(got, plain, err_msg="num %d slab of %d entries" % (num, entries))
                if geodetic:
                    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=0.05)
                else:
                    np.testing.assert_array_equal(got, ref)
            print("distance num %d of %d points, %d locations: slabs of 7, 1 and 400 locations, %.2f s" % (num, n, nq, time.perf_counter() - t0))
    assert (gridpp.distance(sources[N_FROM][0], op, 1)[:20] == 0).all()          # the exact matches
    assert gridpp.active_overrides() == []
