"""GPU: apply_curve (one curve, one curve per cell) and interpolate (vector form) against the float32 restatement of
tests/curve_ref.py, which tests/test_curve_restatement.py pins to the reference's own known answers.

Bit for bit (assert_array_equal, NaNs in the same places), no tolerance and no skipped values: both sides perform the same float32
operations in the same order, the library is built with -ffp-contract=off and correctly rounded division, and no reduction is
involved whose order could differ."""
import itertools

import numpy as np
import pytest

from tests import curve_ref as R

pytestmark = pytest.mark.gpu

PAIRS = list(itertools.product(R.POLICIES, R.POLICIES))
ARRAY_CASES = [c for c in R.CASES if R.needs_device(c)]
LDS_FLOATS = 8192   # CURVE_LDS_FLOATS of gridpp_amd/csrc/curve.hip: both halves of a curve that is staged on chip


@pytest.fixture(scope="module")
def gridpp():
    import gridpp_amd
    if gridpp_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return gridpp_amd


@pytest.mark.parametrize("case", ARRAY_CASES, ids=[c["id"] for c in ARRAY_CASES])
def test_array_form_known_answers(gridpp, case):
    R.check_case(case, gridpp)


def test_the_array_form_cases_are_there():
    fns = [c["function"] for c in ARRAY_CASES]
    assert fns.count("apply_curve") >= 20 and fns.count("interpolate") >= 1


def check_shared(gridpp, rng, n, nc, kind, pairs):
    r, f = R.random_curves(rng, (), nc, kind)
    x = R.random_inputs(rng, (n,), f)
    for pb, pa in pairs:
        got = gridpp.apply_curve(x, r, f, pb, pa)
        assert got.dtype == np.float32 and got.shape == x.shape
        np.testing.assert_array_equal(got, R.apply_curve(x, r, f, pb, pa), err_msg="nc %d %s policies %d %d" % (nc, kind, pb, pa))
    return x, r, f


@pytest.mark.parametrize("kind", ["sorted", "duplicates", "nans", "unsorted", "constant"])
@pytest.mark.parametrize("nc", [1, 2, 3, 10])
def test_shared_curve_small_all_policy_pairs(gridpp, nc, kind):
    rng = np.random.default_rng(100 * nc + len(kind))
    check_shared(gridpp, rng, 1003, nc, kind, PAIRS)


@pytest.mark.parametrize("kind", ["sorted", "duplicates", "nans", "unsorted"])
@pytest.mark.parametrize("nc", [2000, LDS_FLOATS // 2, LDS_FLOATS // 2 + 1, 5000])
def test_shared_curve_long(gridpp, nc, kind):
    """2000: the reference's benchmark row; 4096 / 4097: the last curve staged in LDS and the first read through the caches"""
    rng = np.random.default_rng(nc + len(kind))
    check_shared(gridpp, rng, 20003, nc, kind, [(R.OneToOne, R.MeanSlope), (R.NearestSlope, R.Zero), (R.Unchanged, R.NearestSlope)])


@pytest.mark.parametrize("kind", ["sorted", "unsorted"])
def test_shared_curve_of_a_few_hundred_thousand_entries(gridpp, kind):
    rng = np.random.default_rng(77)
    check_shared(gridpp, rng, 257, 200000, kind, [(R.MeanSlope, R.NearestSlope)])


def test_shared_curve_2d_field_and_tail_lengths(gridpp):
    """a vec2 field keeps its shape; lengths around the 4-value step of the kernel"""
    rng = np.random.default_rng(8)
    r, f = R.random_curves(rng, (), 10, "duplicates")
    x = R.random_inputs(rng, (37, 53), f)
    got = gridpp.apply_curve(x, r, f, R.MeanSlope, R.NearestSlope)
    assert got.shape == (37, 53)
    np.testing.assert_array_equal(got, R.apply_curve(x, r, f, R.MeanSlope, R.NearestSlope))
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 4097):
        x = R.random_inputs(rng, (n,), f)
        np.testing.assert_array_equal(gridpp.apply_curve(x, r, f, R.Zero, R.OneToOne), R.apply_curve(x, r, f, R.Zero, R.OneToOne))


@pytest.mark.parametrize("kind", ["sorted", "duplicates", "nans", "unsorted"])
@pytest.mark.parametrize("nc", [1, 3, 10, 2000, 5000])
def test_interpolate_vector_form(gridpp, nc, kind):
    """incl. its clamp to the end values outside the curve and NaN for an invalid x"""
    rng = np.random.default_rng(31 * nc + len(kind))
    iY, iX = R.random_curves(rng, (), nc, kind)
    x = R.random_inputs(rng, (5001,), iX)
    got = gridpp.interpolate(x, iX, iY)
    want = R.interpolate(x, iX, iY)
    np.testing.assert_array_equal(got, want)
    if kind in ("sorted", "duplicates"):
        assert (got[np.isfinite(x) & (x > iX[-1])] == iY[-1]).all() and (got[np.isfinite(x) & (x < iX[0])] == iY[0]).all()
        assert np.isnan(got[~np.isfinite(x)]).all()


def test_interpolate_empty_curve_gives_nan(gridpp):
    assert np.isnan(gridpp.interpolate(np.arange(7, dtype=np.float32), [], [])).all()


def check_field(gridpp, rng, shape, nc, kinds, pairs):
    r = np.empty(shape + (nc,), np.float32)
    f = np.empty(shape + (nc,), np.float32)
    rows = np.array_split(np.arange(shape[0]), len(kinds))
    for kind, ys in zip(kinds, rows):   # bands of rows, one kind of curve each
        if len(ys):
            r[ys], f[ys] = R.random_curves(rng, (len(ys), shape[1]), nc, kind)
    x = R.random_inputs(rng, shape, f)
    for pb, pa in pairs:
        got = gridpp.apply_curve(x, r, f, pb, pa)
        assert got.dtype == np.float32 and got.shape == x.shape
        np.testing.assert_array_equal(got, R.apply_curve(x, r, f, pb, pa), err_msg="nc %d policies %d %d" % (nc, pb, pa))
    return x, r, f


@pytest.mark.parametrize("nc", [1, 2, 3, 10, 17, 50, 64, 65, 300])
def test_curve_per_cell(gridpp, nc):
    """odd grid shape; sorted / duplicated / NaN-ridden (ends and inside, infinities) / unsorted / constant curves; NaN and
    +-inf inputs.  nc covers the three load widths (4 nc divisible by 16, by 8, by neither), every group size and the chunked loop"""
    rng = np.random.default_rng(1000 + nc)
    pairs = PAIRS if nc in (2, 10, 17) else [(R.OneToOne, R.MeanSlope), (R.MeanSlope, R.NearestSlope), (R.NearestSlope, R.Zero), (R.Zero, R.Unchanged), (R.Unchanged, R.OneToOne)]
    check_field(gridpp, rng, (37, 53), nc, R.KINDS, pairs)


@pytest.mark.parametrize("nc", [1040, 4100])
def test_curve_per_cell_long_runs(gridpp, nc):
    """runs far beyond what a group covers in one step"""
    rng = np.random.default_rng(nc)
    check_field(gridpp, rng, (5, 7), nc, R.KINDS, [(R.MeanSlope, R.NearestSlope)])


def test_curve_per_cell_single_cell_and_single_row(gridpp):
    rng = np.random.default_rng(4)
    for shape in ((1, 1), (1, 9), (9, 1)):
        check_field(gridpp, rng, shape, 10, ("nans",), [(R.NearestSlope, R.MeanSlope)])


def test_float64_host_path_equals_float32_path_on_the_rounded_input(gridpp):
    rng = np.random.default_rng(64)
    r, f = R.random_curves(rng, (), 10, "sorted")
    x64 = rng.normal(0, 1.3, (1 << 20) + 3)
    x64[::1001] = np.nan
    got = gridpp.apply_curve(x64, r, f, R.MeanSlope, R.NearestSlope)
    x32 = x64.astype(np.float32)
    np.testing.assert_array_equal(got, gridpp.apply_curve(x32, r, f, R.MeanSlope, R.NearestSlope))
    np.testing.assert_array_equal(got, R.apply_curve(x32, r, f, R.MeanSlope, R.NearestSlope))
    np.testing.assert_array_equal(gridpp.interpolate(x64, f, r), gridpp.interpolate(x32, f, r))
    # one curve per cell: the curves are the large arrays
    shape = (601, 600)
    r3, f3 = R.random_curves(rng, shape, 3, "sorted")
    x = R.random_inputs(rng, shape, f3)
    got = gridpp.apply_curve(x.astype(np.float64), r3.astype(np.float64), f3.astype(np.float64), R.OneToOne, R.Zero)
    np.testing.assert_array_equal(got, gridpp.apply_curve(x, r3, f3, R.OneToOne, R.Zero))
    np.testing.assert_array_equal(got, R.apply_curve(x, r3, f3, R.OneToOne, R.Zero))


def test_torch_path_returns_a_cuda_tensor_equal_to_the_host_path(gridpp):
    import torch
    rng = np.random.default_rng(9)
    r, f = R.random_curves(rng, (), 50, "duplicates")
    x = R.random_inputs(rng, (101, 203), f)
    want = gridpp.apply_curve(x, r, f, R.NearestSlope, R.MeanSlope)
    xd = torch.from_numpy(x).cuda()
    got = gridpp.apply_curve(xd, r, f, R.NearestSlope, R.MeanSlope)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == x.shape
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    # a view that starts 4 bytes into its buffer (no 16-byte loads there)
    flat = torch.from_numpy(np.concatenate([[0], x.ravel()]).astype(np.float32)).cuda()
    got = gridpp.apply_curve(flat[1:], r, f, R.NearestSlope, R.MeanSlope)
    np.testing.assert_array_equal(got.cpu().numpy(), want.ravel())
    gi = gridpp.interpolate(xd.reshape(-1), f, r)
    assert isinstance(gi, torch.Tensor) and gi.is_cuda
    np.testing.assert_array_equal(gi.cpu().numpy(), gridpp.interpolate(x.ravel(), f, r))
    # one curve per cell, all three fields in HBM; curves of 10 entries are 8-byte, of 64 entries 16-byte aligned per cell
    for nc in (10, 64):
        r3, f3 = R.random_curves(rng, (33, 65), nc, "nans")
        x3 = R.random_inputs(rng, (33, 65), f3)
        want = gridpp.apply_curve(x3, r3, f3, R.MeanSlope, R.Zero)
        got = gridpp.apply_curve(torch.from_numpy(x3).cuda(), torch.from_numpy(r3).cuda(), torch.from_numpy(f3).cuda(), R.MeanSlope, R.Zero)
        assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (33, 65)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        np.testing.assert_array_equal(want, R.apply_curve(x3, r3, f3, R.MeanSlope, R.Zero))
    with pytest.raises(ValueError):   # mixed host / device fields
        gridpp.apply_curve(torch.from_numpy(x3).cuda(), r3, f3, R.MeanSlope, R.Zero)


def test_errors_come_before_device_work_on_the_gpu_box_too(gridpp):
    with pytest.raises(ValueError, match="Unknown extrapolation policy"):
        gridpp.apply_curve([1.0, 2.0], [1, 2], [1, 2], 5, R.OneToOne)
    with pytest.raises(ValueError, match="Unknown extrapolation policy"):   # whatever the data: nothing extrapolates here
        gridpp.apply_curve(np.ones((2, 2)), np.ones((2, 2, 3)), np.ones((2, 2, 3)), R.OneToOne, 7)
    with pytest.raises(ValueError, match="same size"):
        gridpp.apply_curve([1.0], [1, 2], [1, 2, 3], R.OneToOne, R.OneToOne)


def test_full_size_gridded_row_of_the_reference_benchmark(gridpp):
    """2000 x 2000 x 10, curves sorted along the last axis (the reference's tests/benchmark.py "gridded" apply_curve row)"""
    rng = np.random.default_rng(2000)
    shape = (2000, 2000)
    f = np.sort(rng.random(shape + (10,), dtype=np.float32), axis=-1)
    r = np.sort(rng.random(shape + (10,), dtype=np.float32), axis=-1)
    x = rng.uniform(-0.1, 1.1, shape).astype(np.float32)
    got = gridpp.apply_curve(x, r, f, R.OneToOne, R.OneToOne)
    np.testing.assert_array_equal(got, R.apply_curve(x, r, f, R.OneToOne, R.OneToOne))
