"""downscale_probability and mask_threshold_downscale_consensus / _quantile on the device (gridpp_amd/csrc/ensemble_downscale.hip)
against the numpy float32 restatement of tests/ensemble_downscaling_ref.py, which the known answers of the reference's tests pin
(tests/test_ensemble_downscaling_restatement.py).  Everything is bit-exact (assert_array_equal, NaN positions included): the
probability is a ratio of two integer counts, the masked row is reduced in member order by the same float32 expressions as the
oracle's calc_statistic / calc_quantile.  RandomChoice is checked as "one of the valid masked members, NaN iff there is none"."""
import numpy as np
import pytest

from tests import ensemble_downscaling_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
OPS = (R.Lt, R.Leq, R.Gt, R.Geq)
STATS = (R.Mean, R.Min, R.Median, R.Max, R.Std, R.Variance, R.Sum, R.Count)
QUANTILES = (0.0, 0.25, 0.5, 0.9, 1.0, float("nan"))


def row_cap():
    from gridpp_amd import _capi
    return _capi.ENSEMBLE_ROW_CAP   # GPP_ENSEMBLE_ROW_CAP: the longest masked row the kernel stages on chip


# ---- the ten known answers ----------------------------------------------------------------------------------------------------
KNOWN = R.known_answers()


def call_case(gridpp, c, igrid, ogrid, conv=np.asarray):
    op = R.OP_NAMES[c["comparison_operator"]]
    thr = conv(c["threshold"])
    if c["function"] == "downscale_probability":
        return gridpp.downscale_probability(igrid, ogrid, conv(c["values"]), thr, op)
    cubes = [conv(c[k]) for k in ("ivalues_true", "ivalues_false", "threshold_values")]
    if c["function"] == "mask_threshold_downscale_quantile":
        return gridpp.mask_threshold_downscale_quantile(igrid, ogrid, *cubes, thr, op, c["quantile"])
    return gridpp.mask_threshold_downscale_consensus(igrid, ogrid, *cubes, thr, op, R.STAT_NAMES[c["statistic"]])


@pytest.mark.parametrize("case", KNOWN, ids=[c["id"] for c in KNOWN])
def test_known_answer(case):
    import gridpp_amd as gridpp
    g = R.golden()["grids"]
    igrid, ogrid = gridpp.Grid(g["igrid"]["lats"], g["igrid"]["lons"]), gridpp.Grid(g["ogrid"]["lats"], g["ogrid"]["lons"])
    expected = np.asarray(case["expected"], F)
    got = call_case(gridpp, case, igrid, ogrid)
    assert got.dtype == F and got.shape == expected.shape
    np.testing.assert_array_equal(got, expected)
    np.testing.assert_array_equal(call_case(gridpp, case, igrid, ogrid, conv=lambda a: a), expected)   # nested lists in


# ---- randomised cases -----------------------------------------------------------------------------------------------------------
LEVELS = np.array([-1.5, -0.5, 0.0, 0.5, 1.0, 2.5], F)   # few levels: member == threshold is common


class Case:
    """variant: 'finer' (Geodetic, output finer than the input), 'equal' (the same grid), 'coarser' (Cartesian, output coarser)"""

    def __init__(self, E, variant, seed):
        import gridpp_amd as gridpp
        from oracle import oracle as O
        rng = np.random.default_rng(seed)
        Y, X = 7, 9
        if variant == "coarser":
            self.ctype = gridpp.Cartesian
            ilats, ilons = np.meshgrid(np.linspace(0, 60000, Y), np.linspace(-1000, 90000, X), indexing="ij")
            olats, olons = np.meshgrid(np.linspace(-5000, 66000, 4), np.linspace(0, 95000, 5), indexing="ij")
        else:
            self.ctype = gridpp.Geodetic
            ilats, ilons = np.meshgrid(np.linspace(50.0, 52.0, Y), np.linspace(5.0, 8.0, X), indexing="ij")
            if variant == "equal":
                olats, olons = ilats, ilons
            else:
                olats, olons = np.meshgrid(np.linspace(49.9, 52.1, 15), np.linspace(4.9, 8.1, 19), indexing="ij")
        self.igrid, self.ogrid = gridpp.Grid(ilats, ilons, ((),), ((),), self.ctype), gridpp.Grid(olats, olons, ((),), ((),), self.ctype)
        self.idx = O.nearest_indices(O.Pts(ilats.ravel(), ilons.ravel(), ctype=self.ctype), O.Pts(olats.ravel(), olons.ravel(), ctype=self.ctype))
        self.E, self.oshape = E, olats.shape

        def cube(spoil):
            a = LEVELS[rng.integers(0, LEVELS.size, (Y, X, E))]
            if spoil:
                a[rng.random(a.shape) < 0.08] = np.nan
                a[rng.random(a.shape) < 0.03] = np.inf
                a[rng.random(a.shape) < 0.03] = -np.inf
                a[rng.random((Y, X)) < 0.15] = np.nan   # cells with no valid member
            return a
        self.values = cube(True)
        self.vt, self.vf, self.tv = cube(True) * F(3) + F(0.1), cube(True) - F(7), cube(True)
        thr = LEVELS[rng.integers(0, LEVELS.size, self.oshape)]
        flat = thr.reshape(-1)
        n = flat.size
        flat[rng.choice(n, max(1, n // 12), replace=False)] = np.nan
        flat[rng.choice(n, max(1, n // 20), replace=False)] = np.inf
        flat[rng.choice(n, max(1, n // 20), replace=False)] = -np.inf
        self.thr = thr


def members():
    return [1, 2, 3, 50, 51, 64, 100, 257, row_cap() + 1]


VARIANTS = ("finer", "equal", "coarser")
PARAMS = [(E, VARIANTS[i % 3]) for i, E in enumerate([1, 2, 3, 50, 51, 64, 100, 257, "beyond"])] + [(50, "equal"), (50, "coarser"), (3, "finer"),
                                                                                                     (257, "coarser"), (64, "finer")]


def _E(E):
    return row_cap() + 1 if E == "beyond" else E


@pytest.mark.parametrize("E,variant", PARAMS)
def test_probability_bit_exact(E, variant):
    import gridpp_amd as gridpp
    c = Case(_E(E), variant, 11)
    for op in OPS:
        got = gridpp.downscale_probability(c.igrid, c.ogrid, c.values, c.thr, op)
        ref = R.probability(c.idx, c.values, c.thr, op)
        assert got.dtype == F and got.shape == c.oshape
        np.testing.assert_array_equal(got, ref, err_msg="op %d" % op)
    assert np.isnan(ref).any() and (ref == 0).any() and (ref > 0).any()


@pytest.mark.parametrize("E,variant", PARAMS)
def test_mask_bit_exact(E, variant):
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = Case(_E(E), variant, 12)
    for op in OPS:
        for stat in STATS:
            got = gridpp.mask_threshold_downscale_consensus(c.igrid, c.ogrid, c.vt, c.vf, c.tv, c.thr, op, stat)
            ref = R.mask(O, c.idx, c.vt, c.vf, c.tv, c.thr, op, stat)
            assert got.dtype == F and got.shape == c.oshape
            np.testing.assert_array_equal(got, ref, err_msg="op %d statistic %d" % (op, stat))
        for q in QUANTILES:
            got = gridpp.mask_threshold_downscale_quantile(c.igrid, c.ogrid, c.vt, c.vf, c.tv, c.thr, op, q)
            ref = R.mask(O, c.idx, c.vt, c.vf, c.tv, c.thr, op, R.Quantile, q)
            np.testing.assert_array_equal(got, ref, err_msg="op %d quantile %r" % (op, q))
        # consensus with Quantile is quantile 0 (mask_threshold_downscale_consensus.cpp:12-14)
        np.testing.assert_array_equal(gridpp.mask_threshold_downscale_consensus(c.igrid, c.ogrid, c.vt, c.vf, c.tv, c.thr, op, gridpp.Quantile),
                                      R.mask(O, c.idx, c.vt, c.vf, c.tv, c.thr, op, R.Quantile, 0.0))


def test_the_beyond_capacity_case_is_beyond():
    assert members()[-1] > row_cap() >= 257


@pytest.mark.parametrize("E,variant", [(1, "finer"), (3, "equal"), (50, "coarser"), (100, "finer"), ("beyond", "equal")])
def test_random_choice_is_a_valid_masked_member(E, variant):
    import gridpp_amd as gridpp
    c = Case(_E(E), variant, 13)
    for op in OPS:
        got = gridpp.mask_threshold_downscale_consensus(c.igrid, c.ogrid, c.vt, c.vf, c.tv, c.thr, op, gridpp.RandomChoice).ravel()
        rows = R.masked_rows(c.idx, c.vt, c.vf, c.tv, c.thr, op)
        some = np.isfinite(rows).any(axis=1)
        np.testing.assert_array_equal(np.isnan(got), ~some)
        assert some.any() and (~some).any()
        for k in np.nonzero(some)[0]:
            assert got[k] in rows[k][np.isfinite(rows[k])], (k, got[k])


def test_float64_lists_and_device_tensors_give_the_same_bits():
    import torch
    import gridpp_amd as gridpp
    c = Case(50, "finer", 14)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, F)).cuda()
    base_p = gridpp.downscale_probability(c.igrid, c.ogrid, c.values, c.thr, gridpp.Leq)
    base_m = gridpp.mask_threshold_downscale_consensus(c.igrid, c.ogrid, c.vt, c.vf, c.tv, c.thr, gridpp.Gt, gridpp.Mean)
    base_q = gridpp.mask_threshold_downscale_quantile(c.igrid, c.ogrid, c.vt, c.vf, c.tv, c.thr, gridpp.Lt, 0.3)
    for conv in (lambda a: a.astype(np.float64), lambda a: a.tolist(), dev):
        p = gridpp.downscale_probability(c.igrid, c.ogrid, conv(c.values), conv(c.thr), gridpp.Leq)
        m = gridpp.mask_threshold_downscale_consensus(c.igrid, c.ogrid, conv(c.vt), conv(c.vf), conv(c.tv), conv(c.thr), gridpp.Gt, gridpp.Mean)
        q = gridpp.mask_threshold_downscale_quantile(c.igrid, c.ogrid, conv(c.vt), conv(c.vf), conv(c.tv), conv(c.thr), gridpp.Lt, 0.3)
        if conv is dev:
            assert all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in (p, m, q))
            p, m, q = (t.cpu().numpy() for t in (p, m, q))
        np.testing.assert_array_equal(p, base_p)
        np.testing.assert_array_equal(m, base_m)
        np.testing.assert_array_equal(q, base_q)
    with pytest.raises(ValueError, match="either all field arguments"):
        gridpp.downscale_probability(c.igrid, c.ogrid, dev(c.values), c.thr, gridpp.Leq)


def test_large_float64_cubes_take_the_device_cast():
    """cubes of 2^20 elements and more in float64 are uploaded as they are (GPP_HOST_F64) and cast on the device"""
    import gridpp_amd as gridpp
    rng = np.random.default_rng(15)
    Y, X, E = 128, 128, 64
    lats, lons = np.meshgrid(np.linspace(50, 52, Y), np.linspace(5, 8, X), indexing="ij")
    olats, olons = np.meshgrid(np.linspace(50, 52, 200), np.linspace(5, 8, 150), indexing="ij")
    igrid, ogrid = gridpp.Grid(lats, lons), gridpp.Grid(olats, olons)
    cubes = [rng.normal(0, 1, (Y, X, E)) for _ in range(3)]   # float64 values that float32 rounds
    thr = rng.normal(0, 1, olats.shape)
    c32 = [a.astype(F) for a in cubes]
    np.testing.assert_array_equal(gridpp.downscale_probability(igrid, ogrid, cubes[0], thr, gridpp.Geq),
                                  gridpp.downscale_probability(igrid, ogrid, c32[0], thr.astype(F), gridpp.Geq))
    np.testing.assert_array_equal(gridpp.mask_threshold_downscale_consensus(igrid, ogrid, *cubes, thr, gridpp.Leq, gridpp.Std),
                                  gridpp.mask_threshold_downscale_consensus(igrid, ogrid, *c32, thr.astype(F), gridpp.Leq, gridpp.Std))


def test_no_members_and_empty_input_grid():
    import gridpp_amd as gridpp
    c = Case(3, "finer", 16)
    z = np.zeros((7, 9, 0), F)
    assert np.isnan(gridpp.downscale_probability(c.igrid, c.ogrid, z, c.thr, gridpp.Lt)).all()
    assert np.isnan(gridpp.mask_threshold_downscale_consensus(c.igrid, c.ogrid, z, z, z, c.thr, gridpp.Lt, gridpp.Mean)).all()
    np.testing.assert_array_equal(gridpp.mask_threshold_downscale_consensus(c.igrid, c.ogrid, z, z, z, c.thr, gridpp.Lt, gridpp.Count),
                                  np.zeros(c.oshape, F))
    assert np.isnan(gridpp.mask_threshold_downscale_quantile(c.igrid, c.ogrid, z, z, z, c.thr, gridpp.Lt, 0.5)).all()
    empty = gridpp.Grid(np.zeros((0, 0)), np.zeros((0, 0)))
    z = np.zeros((0, 0, 4), F)
    for out in (gridpp.downscale_probability(empty, c.ogrid, z, c.thr, gridpp.Lt),
                gridpp.mask_threshold_downscale_consensus(empty, c.ogrid, z, z, z, c.thr, gridpp.Lt, gridpp.Count),
                gridpp.smart(empty, c.ogrid, np.zeros((0, 0), F), 3, gridpp.BarnesStructure(10000))):
        assert out.shape == c.oshape and np.isnan(out).all()


# ---- a size the oracle cannot walk (its nearest search is brute force) -----------------------------------------------------------
def test_large_case_against_the_composed_device_path():
    """1000 x 800 x 20 -> 4000 x 4000.  `nearest` of the field arange(Y X) gives every output cell's input index exactly
    (800 000 < 2^24); the rest is torch: integer counts for the probability, and for the mask form one member plane added at a
    time in float32 -- the reference's member order, cell by cell."""
    import torch
    import gridpp_amd as gridpp
    Y, X, E, oY, oX = 1000, 800, 20, 4000, 4000
    lats, lons = np.meshgrid(np.linspace(55.0, 64.0, Y, dtype=F), np.linspace(4.0, 16.0, X, dtype=F), indexing="ij")
    olats, olons = np.meshgrid(np.linspace(54.99, 64.01, oY, dtype=F), np.linspace(3.99, 16.01, oX, dtype=F), indexing="ij")
    igrid, ogrid = gridpp.Grid(lats, lons), gridpp.Grid(olats, olons)
    del lats, lons, olats, olons
    g = torch.Generator(device="cuda").manual_seed(17)
    lev = torch.tensor(LEVELS, device="cuda")

    def cube():
        a = lev[torch.randint(0, lev.numel(), (Y, X, E), device="cuda", generator=g)]
        a[torch.rand((Y, X, E), device="cuda", generator=g) < 0.05] = float("nan")
        a[torch.rand((Y, X, E), device="cuda", generator=g) < 0.01] = float("inf")
        a[torch.rand((Y, X), device="cuda", generator=g) < 0.02] = float("nan")
        return a
    vt, vf, tv = cube() * 3 + 0.1, cube() - 7, cube()
    thr = lev[torch.randint(0, lev.numel(), (oY, oX), device="cuda", generator=g)]
    thr[torch.rand((oY, oX), device="cuda", generator=g) < 0.02] = float("nan")
    idx = gridpp.nearest(igrid, ogrid, torch.arange(Y * X, device="cuda", dtype=torch.float32).reshape(Y, X)).reshape(-1).to(torch.int64)
    assert int(idx.min()) == 0 and int(idx.max()) == Y * X - 1
    t = thr.reshape(-1)
    nan = torch.full((oY * oX,), float("nan"), device="cuda")

    def same(got, ref):
        got = got.reshape(-1)
        assert got.dtype == torch.float32 and bool(torch.equal(torch.isnan(got), torch.isnan(ref)))
        assert bool(torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(ref, nan=0.0)))

    cmp = {gridpp.Leq: torch.le, gridpp.Gt: torch.gt}
    for op in (gridpp.Leq, gridpp.Gt):
        count = torch.zeros(oY * oX, dtype=torch.int32, device="cuda")
        total = torch.zeros_like(count)
        for k in range(E):
            m = tv[:, :, k].reshape(-1)[idx]
            ok = torch.isfinite(m)
            count += ok
            total += ok & cmp[op](m, t)
        ref = torch.where(count > 0, total.float() / count.float(), nan)
        same(gridpp.downscale_probability(igrid, ogrid, tv, thr, op), ref)
        assert bool(torch.isnan(ref).any()) and bool((ref > 0).any())
    op = gridpp.Leq
    s = torch.zeros(oY * oX, device="cuda")
    n = torch.zeros(oY * oX, dtype=torch.int32, device="cuda")
    mx = nan.clone()
    for k in range(E):
        tk = tv[:, :, k].reshape(-1)[idx]
        mk = torch.where(torch.le(tk, t), vt[:, :, k].reshape(-1)[idx], vf[:, :, k].reshape(-1)[idx])
        ok = torch.isfinite(tk) & torch.isfinite(mk)
        s = torch.where(ok, s + mk, s)
        n += ok
        mx = torch.where(ok & (torch.isnan(mx) | (mk > mx)), mk, mx)
    some = n > 0
    for stat, ref in ((gridpp.Sum, torch.where(some, s, nan)), (gridpp.Mean, torch.where(some, s / n.float(), nan)), (gridpp.Count, n.float()),
                      (gridpp.Max, mx)):
        same(gridpp.mask_threshold_downscale_consensus(igrid, ogrid, vt, vf, tv, thr, op, stat), ref)
