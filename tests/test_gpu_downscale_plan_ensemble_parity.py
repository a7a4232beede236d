"""The planned ensemble downscalers (DownscalingPlan.downscale_probability / mask_threshold_downscale_consensus / _quantile: the
shared part of gridpp_amd/csrc/ensemble_downscale.hip run with a plan's nearest grid points) against the direct calls on the same
grids, bit for bit, on a Nearest and on a Bilinear plan.  The direct calls are pinned to the oracle by
tests/test_gpu_ensemble_downscaling_parity.py and tests/test_gpu_size_gated_paths.py.  RandomChoice draws anew every call: its result
must be one of the cell's valid masked members (the masked rows restated in numpy, tests/ensemble_downscaling_ref.py)."""
import contextlib
import functools

import numpy as np
import pytest

from gridpp_amd import _capi
from tests import ensemble_downscaling_ref as ER
from tests.test_gpu_downscale_plan_parity import same_bits

pytestmark = pytest.mark.gpu
F = np.float32
ROW_CAP = _capi.ENSEMBLE_ROW_CAP
LEVELS = np.array([-1.5, -0.5, 0.0, 0.5, 1.0, 2.5], F)   # few levels: member == threshold is common
OPS = (ER.Lt, ER.Leq, ER.Gt, ER.Geq)
STATS = (ER.Mean, ER.Min, ER.Median, ER.Max, ER.Std, ER.Variance, ER.Sum, ER.Count)
QUANTILES = (0.0, 0.3, 0.5, 1.0)


class EnsCase:
    """a warped Y x X input grid and an oY x oX output grid that reaches beyond it; cubes of a few levels with missing members, cells
    with no valid member at all, and thresholds with missing and infinite cells"""

    def __init__(self, E, seed, Y=9, X=11, oY=13, oX=10):
        import gridpp_amd as gridpp
        rng = np.random.default_rng(seed)
        j, i = np.meshgrid(np.arange(Y, dtype=float), np.arange(X, dtype=float), indexing="ij")
        ilats, ilons = 55 + 0.015 * (0.3 * i + j) + 1e-5 * i * i, 8 + 0.02 * (i - 0.3 * j) + 2e-5 * i * j
        olats, olons = np.meshgrid(np.linspace(ilats.min() - 0.01, ilats.max() + 0.01, oY), np.linspace(ilons.min() - 0.01, ilons.max() + 0.01, oX),
                                   indexing="ij")
        self.igrid, self.ogrid = gridpp.Grid(ilats, ilons), gridpp.Grid(olats, olons)
        self.oshape, self.E = (oY, oX), E
        # the nearest input cell of every output cell, by the direct call on a field of cell numbers
        self.idx = np.asarray(gridpp.nearest(self.igrid, self.ogrid, np.arange(Y * X, dtype=F).reshape(Y, X))).astype(np.int64).ravel()

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
        self.plans = [gridpp.downscaling_plan(self.igrid, self.ogrid, ds) for ds in (gridpp.Nearest, gridpp.Bilinear)]

    def direct(self, gridpp, op, stat, q=None):
        if stat == ER.Quantile:
            return gridpp.mask_threshold_downscale_quantile(self.igrid, self.ogrid, self.vt, self.vf, self.tv, self.thr, op, q)
        return gridpp.mask_threshold_downscale_consensus(self.igrid, self.ogrid, self.vt, self.vf, self.tv, self.thr, op, stat)

    def planned(self, plan, op, stat, q=None):
        if stat == ER.Quantile:
            return plan.mask_threshold_downscale_quantile(self.vt, self.vf, self.tv, self.thr, op, q)
        return plan.mask_threshold_downscale_consensus(self.vt, self.vf, self.tv, self.thr, op, stat)

    def check_random_choice(self, got, op):
        got = np.asarray(got).ravel()
        rows = ER.masked_rows(self.idx, self.vt, self.vf, self.tv, self.thr, op)
        some = np.isfinite(rows).any(axis=1)
        np.testing.assert_array_equal(np.isnan(got), ~some)
        assert some.any() and (~some).any()   # a cell with no valid member is NaN
        for k in np.nonzero(some)[0]:
            assert got[k] in rows[k][np.isfinite(rows[k])], (k, got[k])


@functools.lru_cache(maxsize=None)
def ens_case(E):
    return EnsCase(E, 100 + E)


@contextlib.contextmanager
def override(gridpp, name, value):
    gridpp.set_path_override(name, str(value))
    try:
        assert name in gridpp.active_overrides()
        yield
    finally:
        gridpp.set_path_override(name, None)


@pytest.mark.parametrize("E", [1, 5, 17, 64, 65, 300])
def test_planned_equals_direct(E):
    """the four operators, every statistic but RandomChoice and four quantiles, on spoiled members and cells with no valid member"""
    import gridpp_amd as gridpp
    c = ens_case(E)
    direct = {("p", op): gridpp.downscale_probability(c.igrid, c.ogrid, c.vt, c.thr, op) for op in OPS}
    combos = [(OPS[(i + s) % 4], stat, None) for i, stat in enumerate(STATS) for s in (0, 1)]
    combos += [(OPS[(i + s) % 4], ER.Quantile, q) for i, q in enumerate(QUANTILES) for s in (0, 2)]
    for op, stat, q in combos:
        direct[op, stat, q] = c.direct(gridpp, op, stat, q)
    assert {op for op, _, _ in combos} == set(OPS)
    mean = direct[OPS[0], ER.Mean, None]
    assert np.isnan(mean).any() and np.isfinite(mean).any()
    for plan in c.plans:
        before = plan.nbytes
        for op in OPS:
            got = plan.downscale_probability(c.vt, c.thr, op)
            assert got.shape == c.oshape and got.dtype == F
            same_bits(got, direct["p", op])
        for op, stat, q in combos:
            same_bits(c.planned(plan, op, stat, q), direct[op, stat, q])
        # a Bilinear plan keeps the nearest grid points of its records after the first such call: 4 bytes per cell, once
        assert plan.nbytes - before in ((0,) if plan.downscaler == gridpp.Nearest else (0, 4 * c.thr.size))
        assert plan.nbytes >= (4 if plan.downscaler == gridpp.Nearest else 20) * c.thr.size
        for op in OPS[:2]:
            c.check_random_choice(plan.mask_threshold_downscale_consensus(c.vt, c.vf, c.tv, c.thr, op, gridpp.RandomChoice), op)


# members per slab -> the slabs the loop makes of the 130 cells with ROW_CAP + 1 members: several and a ragged last one, one cell each
SLABS = [(40 * (ROW_CAP + 1), [40, 40, 40, 10]), (ROW_CAP, [1] * 130)]


@pytest.mark.parametrize("E", [ROW_CAP, ROW_CAP + 1])
def test_both_sides_of_the_row_cap_and_the_slab_loop(E):
    import gridpp_amd as gridpp
    c = ens_case(E)
    nq = c.thr.size
    combos = [(OPS[i % 4], stat, q) for i, (stat, q) in enumerate([(ER.Mean, None), (ER.Median, None), (ER.Count, None), (ER.Std, None),
                                                                    (ER.Quantile, 0.0), (ER.Quantile, 0.3), (ER.Quantile, 1.0)])]
    assert gridpp.active_overrides() == []
    direct = {k: c.direct(gridpp, *k) for k in combos}   # no override: one slab
    for members, cells in SLABS:
        slab = max(1, min(nq, members // (ROW_CAP + 1)))
        assert [min(slab, nq - q0) for q0 in range(0, nq, slab)] == cells
        for plan in c.plans:
            with override(gridpp, "GPP_ENSEMBLE_SLAB", members):
                for k in combos:
                    same_bits(c.planned(plan, *k), direct[k])
                c.check_random_choice(plan.mask_threshold_downscale_consensus(c.vt, c.vf, c.tv, c.thr, ER.Gt, gridpp.RandomChoice), ER.Gt)
                same_bits(plan.downscale_probability(c.tv, c.thr, ER.Leq), gridpp.downscale_probability(c.igrid, c.ogrid, c.tv, c.thr, ER.Leq))
    assert gridpp.active_overrides() == []


def test_empty_input_grid_and_no_members():
    import gridpp_amd as gridpp
    c = ens_case(5)
    none = np.zeros((0, 0, 3), F)
    for ds in (gridpp.Nearest, gridpp.Bilinear):
        # an empty input grid: all missing, Count included -- as the direct calls
        plan = gridpp.downscaling_plan(gridpp.Grid(), c.ogrid, ds)
        same_bits(plan.downscale_probability(none, c.thr, ER.Gt), gridpp.downscale_probability(gridpp.Grid(), c.ogrid, none, c.thr, ER.Gt))
        for stat in (ER.Mean, ER.Count):
            got = plan.mask_threshold_downscale_consensus(none, none, none, c.thr, ER.Gt, stat)
            same_bits(got, gridpp.mask_threshold_downscale_consensus(gridpp.Grid(), c.ogrid, none, none, none, c.thr, ER.Gt, stat))
            assert got.shape == c.oshape and np.all(np.isnan(got))
        # no members: NaN, and 0 for Count
        plan = c.plans[ds]
        zero = np.zeros(c.vt.shape[:2] + (0,), F)
        same_bits(plan.downscale_probability(zero, c.thr, ER.Lt), gridpp.downscale_probability(c.igrid, c.ogrid, zero, c.thr, ER.Lt))
        for stat, value in ((ER.Mean, np.nan), (ER.Count, 0.0)):
            got = plan.mask_threshold_downscale_consensus(zero, zero, zero, c.thr, ER.Lt, stat)
            same_bits(got, gridpp.mask_threshold_downscale_consensus(c.igrid, c.ogrid, zero, zero, zero, c.thr, ER.Lt, stat))
            assert np.array_equal(got, np.full(c.oshape, value, F), equal_nan=True)
        same_bits(plan.mask_threshold_downscale_quantile(zero, zero, zero, c.thr, ER.Lt, 0.5),
                  gridpp.mask_threshold_downscale_quantile(c.igrid, c.ogrid, zero, zero, zero, c.thr, ER.Lt, 0.5))
        # an empty output grid
        plan = gridpp.downscaling_plan(c.igrid, gridpp.Grid(), ds)
        assert plan.downscale_probability(c.vt, np.zeros((0, 0), F), ER.Gt).shape == (0, 0)


def test_device_tensors_and_a_plan_after_the_gradients():
    """one plan serves the whole chain: gradient-corrected members, then probabilities and a consensus field of them"""
    import torch
    import gridpp_amd as gridpp
    c = ens_case(17)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    for plan in c.plans:
        got = plan.downscale_probability(dev(c.vt), dev(c.thr), ER.Geq)
        assert got.is_cuda and got.dtype == torch.float32
        same_bits(got.cpu().numpy(), gridpp.downscale_probability(c.igrid, c.ogrid, c.vt, c.thr, ER.Geq))
        got = plan.mask_threshold_downscale_quantile(dev(c.vt), dev(c.vf), dev(c.tv), dev(c.thr), ER.Lt, 0.3)
        same_bits(got.cpu().numpy(), c.direct(gridpp, ER.Lt, ER.Quantile, 0.3))
        with pytest.raises(ValueError):
            plan.downscale_probability(dev(c.vt), c.thr, ER.Geq)
        fine = plan.full_gradient_cube(c.vt, [], [])
        assert fine.shape == c.oshape + (17,)
        same_bits(plan.downscale_probability(c.vt, c.thr, ER.Gt), gridpp.downscale_probability(c.igrid, c.ogrid, c.vt, c.thr, ER.Gt))
