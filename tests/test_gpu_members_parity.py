"""GPU: neighbourhood_members and calc_gradient_members on cubes with E of 1, odd, 50 and beyond a wave, X * E no multiple of 4
or 64 or the fused form's strip, fields narrower and shorter than the window, more rows than one strip of the column pass or one row segment of
the fused form, more cells than one segment of the row pass, halfwidth * E on both sides of the fused form's limit of 1024, at halfwidths from 0 to beyond the whole field, with a NaN block, sprinkled NaN, a block missing in every member, +-Inf and a member that is
entirely NaN.

1. exact data (tests/members_ref.py: every sum exact in double, every mean far from a rounding boundary), bit for bit, no cell left out: against
   the numpy restatement, and against the direct neighbourhood / calc_gradient of every plane;
2. general data against the oracle per plane, within the bounds of the 2-D parity tests;
3. every forced form (the two-pass form, band heights, row segments of the fused form) gives the bits of the default one;
4. device tensors, a misaligned device view and a float64 cube give the bits of the float32 numpy call.
The kernels keep no state between calls (their workspaces are borrowed from the staging pool per call), so there is no poisoned rerun."""
import functools

import numpy as np
import pytest

from tests import members_ref as R
from tests.test_gpu_neighbourhood_parity import close

pytestmark = pytest.mark.gpu
F = np.float32
STATS = ["Mean", "Sum", "Count", "Min", "Max", "Std", "Variance"]
EXACT_SHAPES = R.SHAPES + [(6, 5, 64)]     # halfwidth * E = 1024 at halfwidth 16: the last halo the fused form takes, 17 is the two-pass form's
GRADIENT_CASES = [(1, 0, np.nan, -0.0065), (3, 5, 100.0, 0.0), (7, 2, 0.0, 1.0)]   # tests/test_gpu_gridops_parity.py::test_calc_gradient_matches_oracle


def same_bits(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == F and b.dtype == F, what
    assert (np.isnan(a) == np.isnan(b)).all(), (what, int(np.isnan(a).sum()), int(np.isnan(b).sum()))
    m = ~np.isnan(b)
    bad = a[m].view(np.uint32) != b[m].view(np.uint32)
    # (+0 and -0 are different bits: a sum that cancels is +0 in every summation order under round-to-nearest)
    assert not bad.any(), (what, int(bad.sum()), a[m][bad][:4], b[m][bad][:4])


def seed(shape):
    return shape[0] * 10007 + shape[1] * 101 + shape[2]


@functools.lru_cache(maxsize=None)
def exact(shape):
    return R.exact_cube(seed(shape), shape)


@functools.lru_cache(maxsize=None)
def general(shape):
    return R.general_cube(seed(shape) + 1, shape)


@functools.lru_cache(maxsize=None)
def exact_bases(shape):
    """a shared (Y, X) base and a (Y, X, E) base per member, exact data with invalid values of their own"""
    rng = np.random.default_rng(7)
    shared = (rng.integers(-512, 513, shape[:2]) / 8).astype(F)
    shared[rng.random(shape[:2]) < 0.05] = np.nan
    shared[0, 0] = np.inf
    per = R.exact_cube(seed(shape) + 2, shape)
    return shared, per


@functools.lru_cache(maxsize=None)
def general_gradient_case(shape):
    """the recipe of tests/test_gpu_gridops_parity.py::test_calc_gradient_matches_oracle, per member"""
    rng = np.random.default_rng(23)
    Y, X, E = shape
    base = rng.uniform(0, 1500, (Y, X)).astype(F)
    values = (280 - 0.0065 * base[:, :, None] + rng.normal(0, 0.3, shape)).astype(F)
    base[Y // 3:Y // 3 + max(1, Y // 6), X // 7:X // 7 + max(1, X // 2)] = np.nan
    values[rng.random(shape) < 0.03] = np.nan
    if E > 1:
        values[:, :, E // 2] = np.nan
    return base, values


@pytest.fixture(scope="module")
def gridpp():
    import gridpp_amd
    return gridpp_amd


# ---- 1. exact data, bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", R.HALFWIDTHS)
@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_exact_data_against_the_restatement_and_the_direct_call(gridpp, shape, hw):
    cube = exact(shape)
    assert np.isnan(cube).any() and np.isinf(cube).any() and (shape[2] == 1 or np.isnan(cube[:, :, shape[2] // 2]).all())
    for name in STATS:
        stat = getattr(gridpp, name)
        got = gridpp.neighbourhood_members(cube, hw, stat)
        assert isinstance(got, np.ndarray) and got.dtype == F and got.shape == shape
        if name not in ("Std", "Variance"):
            same_bits(got, R.expected(cube, hw, name), "%s vs the restatement" % name)
        same_bits(got, R.per_plane(gridpp.neighbourhood, cube, hw, stat), "%s vs neighbourhood(plane)" % name)
    count = gridpp.neighbourhood_members(cube, hw, gridpp.Count)
    assert not np.isnan(count).any()                                # Count is never NaN ...
    assert count.min() == 0 or hw > 0                               # ... and 0 where the window holds no valid value


@pytest.mark.parametrize("per_member_base", [False, True])
@pytest.mark.parametrize("gradient_type", ["MinMax", "LinearRegression"])
@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_exact_gradients_against_the_direct_call(gridpp, shape, gradient_type, per_member_base):
    values = exact(shape)
    shared, per = exact_bases(shape)
    base = per if per_member_base else shared
    gt = getattr(gridpp, gradient_type)
    cases = GRADIENT_CASES + [(hw, 2, np.nan, 0.0) for hw in R.HALFWIDTHS if hw not in (0, 1, 7)]
    differs = False
    for hw, num_min, min_range, dflt in cases:
        got = gridpp.calc_gradient_members(base, values, gt, hw, num_min, min_range, dflt)
        assert isinstance(got, np.ndarray) and got.dtype == F and got.shape == shape
        want = np.stack([np.asarray(gridpp.calc_gradient(np.ascontiguousarray(base[:, :, e]) if per_member_base else shared,
                                                         np.ascontiguousarray(values[:, :, e]), gt, hw, num_min, min_range, dflt)) for e in range(shape[2])], -1)
        same_bits(got, want, "%s hw %d" % (gradient_type, hw))
        with np.errstate(invalid="ignore"):
            differs |= bool((got != F(dflt)).any())
    assert differs                                                     # not every cell took the default


# ---- 2. general data against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", R.HALFWIDTHS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_general_data_against_the_oracle(gridpp, shape, hw):
    from oracle import oracle as O
    cube = general(shape)
    ref = {name: R.per_plane(O.neighbourhood, cube, hw, getattr(O, name)) for name in STATS}
    got = {name: gridpp.neighbourhood_members(cube, hw, getattr(gridpp, name)) for name in STATS}
    close(got["Mean"], ref["Mean"])
    close(got["Sum"], ref["Sum"])
    for name in ("Count", "Min", "Max"):
        close(got[name], ref[name], exact=True)
    ex2 = R.mean_of_squares(cube, hw)
    ok = ~np.isnan(ref["Variance"])
    assert (np.isnan(got["Variance"]) == ~ok).all()
    err = np.abs(got["Variance"][ok].astype(np.float64) - ref["Variance"][ok])
    bound = 1e-5 * ex2[ok] + 1e-9
    print("variance hw %d: max err / bound = %.3g" % (hw, (err / bound).max()))
    assert (err <= bound).all(), (err / bound).max()
    if hw > 0:      # (a window of one cell has no variance to speak of)
        well = ok & (ref["Variance"] >= 0.05 * ex2)
        assert well.sum() > 0.5 * ok.sum(), (well.sum(), ok.sum())
        rel = np.abs(got["Std"][well].astype(np.float64) - ref["Std"][well]) / ref["Std"][well]
        print("std hw %d: max rel err = %.3g on %d of %d cells" % (hw, rel.max(), well.sum(), ok.sum()))
        assert rel.max() < 1e-5, rel.max()


@pytest.mark.parametrize("gradient_type", ["MinMax", "LinearRegression"])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_general_gradients_against_the_oracle(gridpp, shape, gradient_type):
    from oracle import oracle as O
    base, values = general_gradient_case(shape)
    gt = getattr(gridpp, gradient_type)
    for hw, num_min, min_range, dflt in GRADIENT_CASES + [(16, 2, np.nan, 0.0), (40, 2, np.nan, 0.0)]:
        got = gridpp.calc_gradient_members(base, values, gt, hw, num_min, min_range, dflt)
        ref = R.per_plane(lambda plane: O.calc_gradient(base, plane, gt, hw, num_min, min_range, dflt), values)
        if gradient_type == "MinMax":
            np.testing.assert_array_equal(got, ref)
        else:
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-6)


# ---- 3. forms ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 29, 5), (130, 3, 1), (33, 65, 50), (6, 5, 64)])
def test_every_forced_form_gives_the_same_bits(gridpp, shape):
    """GPP_MEMBERS_TWO_PASS: the two-pass form where the fused one is the default (halfwidth * E <= 1024; at 40 * 50 and 17 * 64 the default is the
    two-pass form already).  GPP_MEMBERS_BAND_ROWS: bands of one row, of less than a strip of the column pass, of a strip and a row, against the
    default (one band at these sizes).  GPP_MEMBERS_SEG_ROWS: the row segments of the fused form, shorter and longer than the default 16."""
    cube = exact(shape)
    shared, _ = exact_bases(shape)
    lr = gridpp.LinearRegression

    def results():
        out = {(name, hw): gridpp.neighbourhood_members(cube, hw, getattr(gridpp, name)) for name in STATS for hw in (0, 7, 16, 17, 40)}
        out["gradient"] = gridpp.calc_gradient_members(shared, cube, lr, 3, 2, np.nan, 0.0)
        return out
    assert not [n for n in gridpp.active_overrides() if n.startswith("GPP_MEMBERS")]
    want = results()
    settings = [{"GPP_MEMBERS_TWO_PASS": 1}, {"GPP_MEMBERS_SEG_ROWS": 5}, {"GPP_MEMBERS_SEG_ROWS": 64}]
    settings += [dict(two_pass, GPP_MEMBERS_BAND_ROWS=rows) for rows in (1, 5, 32, 33) for two_pass in ({}, {"GPP_MEMBERS_TWO_PASS": 1})]
    for setting in settings:
        try:
            for name, value in setting.items():
                gridpp.set_path_override(name, value)
            got = results()
        finally:
            for name in setting:
                gridpp.set_path_override(name, None)
        for key in want:
            same_bits(got[key], want[key], "%s, %s" % (setting, key))


# ---- 4. layout ----------------------------------------------------------------------------------------------------------------------------------
def test_device_tensors_misaligned_views_and_float64(gridpp):
    import torch
    shape = (37, 29, 5)
    cube = exact(shape)
    shared, per = exact_bases(shape)
    dev = torch.device("cuda:0")
    d_cube, d_shared, d_per = torch.from_numpy(cube).to(dev), torch.from_numpy(shared).to(dev), torch.from_numpy(per).to(dev)
    store = torch.empty(cube.size + 1, dtype=torch.float32, device=dev)
    store[1:] = d_cube.reshape(-1)
    off = store[1:].view(shape)                                                     # one float past an aligned address
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    bstore = torch.empty(shared.size + 1, dtype=torch.float32, device=dev)
    bstore[1:] = d_shared.reshape(-1)
    boff = bstore[1:].view(shape[:2])
    for hw in (1, 16):
        for name in STATS:
            stat = getattr(gridpp, name)
            want = gridpp.neighbourhood_members(cube, hw, stat)
            got = gridpp.neighbourhood_members(d_cube, hw, stat)
            assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == shape
            same_bits(got.cpu().numpy(), want, "device %s" % name)
            same_bits(gridpp.neighbourhood_members(off, hw, stat).cpu().numpy(), want, "misaligned %s" % name)
            same_bits(gridpp.neighbourhood_members(cube.astype(np.float64), hw, stat), want, "float64 %s" % name)
        for gt in (gridpp.MinMax, gridpp.LinearRegression):
            for b, d_b in ((shared, d_shared), (per, d_per)):
                want = gridpp.calc_gradient_members(b, cube, gt, hw)
                got = gridpp.calc_gradient_members(d_b, d_cube, gt, hw)
                assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == shape
                same_bits(got.cpu().numpy(), want, "device gradient")
                same_bits(gridpp.calc_gradient_members(b.astype(np.float64), cube.astype(np.float64), gt, hw), want, "float64 gradient")
            same_bits(gridpp.calc_gradient_members(boff, off, gt, hw).cpu().numpy(), gridpp.calc_gradient_members(shared, cube, gt, hw), "misaligned gradient")
    with pytest.raises(ValueError):
        gridpp.calc_gradient_members(shared, d_cube, gridpp.MinMax, 1)            # host and device fields do not mix


def test_alternating_shapes_and_statistics(gridpp):
    """a sequence in which a buffer of the previous call is larger, smaller and of another kind than the next one needs: every result equals
    the first one computed for its case"""
    cases = [((33, 65, 50), 15, "Mean"), ((9, 70, 3), 40, "Max"), ((37, 29, 5), 7, "Std"), ((130, 3, 1), 1, "Count"), ((5, 4, 65), 16, "Min"),
             ((33, 65, 50), 1, "Variance"), ((9, 70, 3), 0, "Sum")]
    first = {}
    for rep in range(2):
        for shape, hw, name in cases if rep == 0 else cases[::-1]:
            got = gridpp.neighbourhood_members(exact(shape), hw, getattr(gridpp, name))
            grad = gridpp.calc_gradient_members(exact_bases(shape)[0], exact(shape), gridpp.LinearRegression, max(hw, 1))
            if rep == 0:
                first[(shape, hw, name)] = (got, grad)
            else:
                same_bits(got, first[(shape, hw, name)][0], name)
                same_bits(grad, first[(shape, hw, name)][1], "gradient")
        gridpp.release_workspaces()
