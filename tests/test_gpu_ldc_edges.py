"""local_distribution_correction on the device (gridpp_amd/csrc/ldc.hip) at its count, trim and zero-rho edges: the fixtures of
tests/ldc_edge_cases.py (tests/test_ldc_edge_cases_oracle.py shows on the CPU that they reach what they claim) against the restatement of
tests/ldc_ref.py, by the comparison rule of tests/test_gpu_ldc_parity.py, unchanged: every cell that does not take branch 4 bit for
bit, NaN where the restatement has NaN, branch-4 cells within 1e-5 max(|ref|, 1e-3); no cell is exempt.

The one free quantity is the order of the float32 sum of rho (the restatement adds in the order of enumeration, the device in sorted order).
On the ladder, shuffling that order in the restatement moved the branch-4 results by at most 0.018 of the bound (measured on the CPU), so
the bound is the project's parity tolerance and not an allowance for anything else.  Every test prints max err / bound; measured on the
MI355X: at most 0.0152 on the tie-free ladder and 0.228 on the rounded one (one cell whose result is w1 b with w1 = 1 - w0 = 0.0266: one
last-bit step of w0 is 0.224 of the bound), both reproduced to the digit on the CPU by summing rho in the device's order.

Every way of running a fixture -- the default dispatch, every cell on the HBM path (GPP_LDC_HBM), the keys filled in passes of at most
1 000 or 300 pairs (GPP_CSR_CAP), host arrays or device tensors, a sub-grid, the stations in another order -- must give the same bits."""
import functools

import numpy as np
import pytest

from tests import ldc_edge_cases as K
from tests import ldc_ref as R
from tests.test_gpu_ldc_parity import check

pytestmark = pytest.mark.gpu
F = np.float32
QUANTILES = tuple(K.LADDER_QUANTILES)


@functools.lru_cache(maxsize=None)
def handles(fx):
    import gridpp_amd as gridpp
    return fx.device(gridpp)


def run(fx, minq=None, maxq=None, tensors=False):
    import gridpp_amd as gridpp
    grid, points, st = handles(fx)
    fields = [np.array(a) for a in (fx.bg, fx.pobs, fx.pbg)]
    if tensors:
        import torch
        fields = [torch.from_numpy(a).cuda() for a in fields]
    got = gridpp.local_distribution_correction(grid, fields[0], points, fields[1], fields[2], st, fx.minq if minq is None else minq,
                                               fx.maxq if maxq is None else maxq, fx.min_points)
    if tensors:
        assert got.is_cuda
        got = got.cpu().numpy()
    return got


@functools.lru_cache(maxsize=None)
def full_ladder(rounded, q):
    """the full ladder by the default dispatch: what every other way of running it is compared with (computed once, read-only)"""
    got = run(K.ladder(rounded), *q)
    got.setflags(write=False)
    return got


def same_bits(a, b):
    np.testing.assert_array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("q", QUANTILES, ids=lambda q: "q%g-%g" % q)
@pytest.mark.parametrize("rounded", [False, True], ids=["tiefree", "rounded"])
def test_ladder(rounded, q, monkeypatch):
    """counts 1 ... 2 049 in one call: both finishing kernels launched with cells for each, 300 cells"""
    import gridpp_amd as gridpp
    fx = K.ladder(rounded)
    ref, tags, counts, _ = fx.restate(*q)
    assert counts.max() > K.LDS_MAX and (counts <= K.LDS_MAX).any()
    base = full_ladder(rounded, q)
    check(base, ref, tags)
    monkeypatch.setenv("GPP_LDC_HBM", "1")
    hbm = run(fx, *q)
    assert "GPP_LDC_HBM" in gridpp.active_overrides()
    check(hbm, ref, tags)
    same_bits(hbm, base)
    monkeypatch.delenv("GPP_LDC_HBM")
    for cap in K.LADDER_CAPS:   # the 1 023+ cells in passes of their own; pass borders between LDS-sized and HBM-sized cells
        monkeypatch.setenv("GPP_CSR_CAP", str(cap))
        chunked = run(fx, *q)
        assert "GPP_CSR_CAP" in gridpp.active_overrides()
        check(chunked, ref, tags)
        same_bits(chunked, base)
    monkeypatch.delenv("GPP_CSR_CAP")


@pytest.mark.parametrize("q", [(0.0, 1.0), (0.1, 0.9), (0.3, 0.31)], ids=lambda q: "q%g-%g" % q)
def test_column_subsets(q):
    """only the columns up to 512 pairs (the HBM kernel is never launched); those and the 513 column (launched for ten cells); one row of
    those (launched for a single cell): the same bits as in the full ladder"""
    full = K.ladder(True)
    subsets = (K.ladder(True, K.ladder_columns(K.LDS_MAX)), K.ladder(True, K.ladder_columns(K.LDS_MAX + 1)),
               K.ladder(True, K.ladder_columns(K.LDS_MAX + 1), rows=(4,)))
    assert [int((s.counts > K.LDS_MAX).sum() * len(s.rows)) for s in subsets] == [0, 10, 1]
    for sub in subsets:
        got = run(sub, *q)
        ref, tags, _, _ = sub.restate(*q)
        check(got, ref, tags)
        same_bits(got, K.sub_grid(full_ladder(True, q), sub))


@pytest.mark.parametrize("q", [(0.0, 1.0), (0.1, 0.9)], ids=lambda q: "q%g-%g" % q)
def test_station_permutation(q, monkeypatch):
    """rounded values: the tie rule holds on the bitonic network and on the radix sort, whatever order the neighbours are met in"""
    fx, perm = K.ladder(True), K.ladder(True, permuted=True)
    ref, tags, _, _ = fx.restate(*q)
    got = run(perm, *q)
    check(got, ref, tags)
    same_bits(got, full_ladder(True, q))
    monkeypatch.setenv("GPP_LDC_HBM", "1")
    same_bits(run(perm, *q), full_ladder(True, q))


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", K.ZERO_RHO)
def test_zero_rho(case, tensors, monkeypatch):
    fx = K.zero_rho(case)
    ref, tags, _, sums = fx.restate()
    assert tags[0] == R.B4 and (sums["sum_r"][0] == 0 or sums["sum_f"][0] == 0) and np.isnan(ref.ravel()[0])
    got = run(fx, tensors=tensors)
    check(got, ref, tags)
    monkeypatch.setenv("GPP_LDC_HBM", "1")
    same_bits(run(fx, tensors=tensors), got)


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "device"])
def test_thresholds(tensors, monkeypatch):
    fx = K.thresholds()
    ref, tags, _, _ = fx.restate()
    got = run(fx, tensors=tensors)
    check(got, ref, tags)
    monkeypatch.setenv("GPP_LDC_HBM", "1")
    same_bits(run(fx, tensors=tensors), got)


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", ["Barnes", "Linear"])
def test_membership(kind, tensors):
    import gridpp_amd as gridpp
    fx = K.membership(kind)
    ref, tags, counts, _ = fx.restate()
    assert list(counts) == ([6, 0] if kind == "Barnes" else [0, 0])
    _, _, st = handles(fx)
    assert st.localization_distance() == fx.oracle_structure.localization_distance() == (5000.0 if kind == "Barnes" else 0.0)
    check(run(fx, tensors=tensors), ref, tags)
