"""calc_quantile / calc_statistic on device-resident arrays, and the four selection paths of gridpp_amd/csrc/rows_select.hip (lane, tile,
block, split: forced with GPP_ROWS_SELECT where their preconditions hold, and the default dispatch), against the numpy restatement of
the result contract (tests/rows_select_ref.py, itself held to the CPU oracle by tests/test_rows_select_restatement.py): bit for bit, the
sign of a zero included."""
import contextlib
import functools

import numpy as np
import pytest

from tests import rows_select_ref as ref
from tests.test_gpu_neighbourhood_edges import QUANTILES, bit_equal, members, rows
from tests.test_gpu_neighbourhood_parity import close

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 159, 160, 161, 255, 256, 257, 1000, 4097]
ROW_COUNTS = [1, 63, 64, 65, 70, 129]          # full tiles of 64 rows, a partial last tile, a single row
PATHS = [None, "lane", "tile", "block", "split"]
SCALAR_Q = 0.9
FIELD_Q = np.array(QUANTILES + [0.25, 0.9, 0.5, 1.0, 0.0], np.float32)   # 0, 1, NaN and interior levels, mixed along the rows


@pytest.fixture(scope="module")
def api():
    import torch
    import gridpp_amd as gridpp
    from oracle import oracle as O
    return gridpp, O, torch


@contextlib.contextmanager
def forced(gridpp, path):
    if path is not None:
        gridpp.set_path_override("GPP_ROWS_SELECT", path)
    try:
        yield
    finally:
        gridpp.set_path_override("GPP_ROWS_SELECT", None)


@functools.lru_cache(maxsize=None)
def base(L):
    a = np.concatenate([rows(L), ref.adversarial(L)])
    a.setflags(write=False)
    return a


def data(L, R):
    b = base(L)
    return np.ascontiguousarray(b[np.arange(R) % b.shape[0]])


def field_q(R):
    return FIELD_Q[(np.arange(R) * 5) % FIELD_Q.size]


@functools.lru_cache(maxsize=None)
def want(L, R, per_row):
    """the restatement's answer, computed once per shape and shared by the paths"""
    w = ref.rows_quantile(data(L, R), field_q(R) if per_row else SCALAR_Q)
    w.setflags(write=False)
    return w


def identical(got, expect):
    got, expect = np.asarray(got, np.float32).ravel(), np.asarray(expect, np.float32).ravel()
    assert got.shape == expect.shape
    ng, ne = np.isnan(got), np.isnan(expect)
    assert (ng == ne).all(), np.nonzero(ng != ne)[0][:5]
    diff = (got.view(np.uint32) != expect.view(np.uint32)) & ~ng
    assert not diff.any(), (np.nonzero(diff)[0][:5], got[diff][:5], expect[diff][:5])


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("path", PATHS)
def test_every_path(api, path, L):
    """a scalar level and a per-row field of levels, on every row count, through one path (None: the default dispatch)"""
    gridpp, O, torch = api
    with forced(gridpp, path):
        for R in ROW_COUNTS:
            t = torch.from_numpy(data(L, R)).cuda()
            identical(gridpp.calc_quantile(t, SCALAR_Q).cpu().numpy(), want(L, R, False))
            q = torch.from_numpy(field_q(R).reshape(R, 1)).cuda()
            identical(gridpp.calc_quantile(t.reshape(R, 1, L), q).cpu().numpy(), want(L, R, True))


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("path", [None, "split"])
def test_split_path_on_long_rows(api, path, R):
    """rows of 70 001 values: the default dispatch takes several workgroups per row here"""
    gridpp, O, torch = api
    L = 70001
    rng = np.random.default_rng(R)
    a = rng.normal(280, 15, (R, L)).astype(np.float32)
    a[:, ::97] = np.nan
    a[R - 1, 5::1001] = np.inf
    a[0, 7] = -0.0
    levels = np.array([0.5, 0.0, 1.0], np.float32)[:R]
    t = torch.from_numpy(a).cuda()
    with forced(gridpp, path):
        for q in (0.5, 0.999, 0.0, 1.0):
            identical(gridpp.calc_quantile(t, q).cpu().numpy(), ref.rows_quantile(a, q))
        got = gridpp.calc_quantile(t.reshape(R, 1, L), torch.from_numpy(levels.reshape(R, 1)).cuda())
        identical(got.cpu().numpy(), ref.rows_quantile(a, levels))
        assert isinstance(gridpp.calc_quantile(t[0], 0.95), float)
        identical([gridpp.calc_quantile(t[0], 0.95)], [ref.quantile(a[0], 0.95)])


@pytest.mark.parametrize("L", [4, 50, 160])
def test_unaligned_input(api, L):
    """a view that starts one float into a buffer gives the bits of the aligned copy"""
    gridpp, O, torch = api
    R = 70
    a = data(L, R)
    buf = torch.empty(R * L + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(R, L)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4
    aligned = torch.from_numpy(a).cuda()
    q = torch.from_numpy(field_q(R).reshape(R, 1)).cuda()
    for path in (None, "tile"):
        with forced(gridpp, path):
            for t in (view, aligned):
                identical(gridpp.calc_quantile(t, SCALAR_Q).cpu().numpy(), want(L, R, False))
                identical(gridpp.calc_quantile(t.view(R, 1, L), q).cpu().numpy(), want(L, R, True))
                identical(gridpp.calc_statistic(t, gridpp.Median).cpu().numpy(), ref.rows_quantile(a, 0.5))


@pytest.mark.parametrize("L", [5, 160, 1000])
def test_host_and_device_input_agree(api, L):
    gridpp, O, torch = api
    R = 70
    a = data(L, R)
    t = torch.from_numpy(a).cuda()
    for q in QUANTILES:
        identical(gridpp.calc_quantile(t, q).cpu().numpy(), gridpp.calc_quantile(a, q))
    q2 = field_q(R).reshape(7, 10)
    host = gridpp.calc_quantile(a.reshape(7, 10, L), q2)
    identical(gridpp.calc_quantile(t.reshape(7, 10, L), torch.from_numpy(q2).cuda()).cpu().numpy(), host)
    identical(gridpp.calc_quantile(t.reshape(7, 10, L), q2).cpu().numpy(), host)   # a host field beside a device cube is uploaded
    identical(host, want(L, R, True))
    for stat in (gridpp.Mean, gridpp.Median, gridpp.Std):
        identical(gridpp.calc_statistic(t, stat).cpu().numpy(), gridpp.calc_statistic(a, stat))


def test_return_types_and_devices(api):
    gridpp, O, torch = api
    a = data(50, 70)
    t = torch.from_numpy(a).cuda()
    s = gridpp.calc_quantile(t[0], 0.5)
    assert isinstance(s, float) and s == gridpp.calc_quantile(a[0], 0.5)
    s = gridpp.calc_statistic(t[0], gridpp.Mean)
    assert isinstance(s, float) and s == gridpp.calc_statistic(a[0], gridpp.Mean)
    for out in (gridpp.calc_quantile(t, 0.5), gridpp.calc_statistic(t, gridpp.Max)):
        assert isinstance(out, torch.Tensor) and out.device == t.device and out.dtype == torch.float32 and tuple(out.shape) == (70,)
    out = gridpp.calc_quantile(t.reshape(7, 10, 50), torch.full((7, 10), 0.5, device="cuda"))
    assert isinstance(out, torch.Tensor) and out.device == t.device and tuple(out.shape) == (7, 10)
    assert isinstance(gridpp.calc_quantile(a, 0.5), np.ndarray) and isinstance(gridpp.calc_statistic(a, gridpp.Max), np.ndarray)
    with pytest.raises(ValueError, match="either all field arguments"):   # a device-resident level beside a host array
        gridpp.calc_quantile(a.reshape(7, 10, 50), torch.full((7, 10), 0.5, device="cuda"))


@pytest.mark.parametrize("L", [5, 160, 161, 1000])
def test_calc_statistic_on_tensors(api, L):
    """the eight statistics per row against the oracle, as test_long_rows does for arrays (the Median's zero may have either sign there:
    std::sort); the Median also against the restatement, exactly"""
    gridpp, O, torch = api
    a = rows(L)
    t = torch.from_numpy(a).cuda()
    for stat in (gridpp.Mean, gridpp.Sum, gridpp.Count, gridpp.Min, gridpp.Max, gridpp.Std, gridpp.Variance, gridpp.Median):
        got = gridpp.calc_statistic(t, stat).cpu().numpy()
        bit_equal(got, [O.calc_statistic(r, stat) for r in a], zero_sign=stat == gridpp.Median)
    identical(gridpp.calc_statistic(t, gridpp.Median).cpu().numpy(), ref.rows_quantile(a, 0.5))
    for stat in (gridpp.Quantile, gridpp.RandomChoice):
        with pytest.raises(RuntimeError):
            gridpp.calc_statistic(t, stat)


def test_errors_and_empty_shapes(api):
    gridpp, O, torch = api
    a = data(50, 70)
    t = torch.from_numpy(a).cuda()
    msg = "Quantile must be between 0 and 1 inclusive"
    for bad in (1.5, -0.1):
        with pytest.raises(ValueError, match=msg):
            gridpp.calc_quantile(t, bad)
        with pytest.raises(ValueError, match=msg):
            gridpp.calc_quantile(t[0], bad)
    q = np.full((7, 10), 0.5, np.float32)
    q[3, 4] = 1.0001
    with pytest.raises(ValueError, match=msg):
        gridpp.calc_quantile(t.reshape(7, 10, 50), torch.from_numpy(q).cuda())
    q[3, 4] = np.nan                                         # NaN passes, and gives NaN
    got = gridpp.calc_quantile(t.reshape(7, 10, 50), torch.from_numpy(q).cuda()).cpu().numpy()
    identical(got, ref.rows_quantile(a, q.ravel()))
    assert np.isnan(got[3, 4])
    for shape in ((7, 9), (10, 7), (70,)):
        with pytest.raises(ValueError, match="Dimension mismatch between array and quantile"):
            gridpp.calc_quantile(t.reshape(7, 10, 50), torch.full(shape, 0.5, device="cuda"))
    with pytest.raises(ValueError, match="Dimension mismatch between array and quantile"):   # the size check comes before the range check
        gridpp.calc_quantile(t.reshape(7, 10, 50), torch.full((7, 9), 1.5, device="cuda"))
    none = torch.empty((0, 5), device="cuda")
    assert tuple(gridpp.calc_quantile(none, 0.5).shape) == (0,) and tuple(gridpp.calc_statistic(none, gridpp.Median).shape) == (0,)
    empty = torch.empty((3, 0), device="cuda")
    for out in (gridpp.calc_quantile(empty, 0.5), gridpp.calc_statistic(empty, gridpp.Median)):
        assert tuple(out.shape) == (3,) and bool(torch.isnan(out).all())
    with pytest.raises(RuntimeError):
        gridpp.calc_quantile(torch.empty((2, 2, 2, 2), device="cuda"), 0.5)


@pytest.mark.parametrize("E", [1, 3, 50, 160, 161])
def test_cube_median_through_the_new_path(api, E):
    """neighbourhood(cube, hw, Median): the member Median of 37 x 29 cells (the last tile of 64 holds 49) comes from rows_select.hip"""
    gridpp, O, torch = api
    f = members(300 + E, 37, 29, E)
    t = torch.from_numpy(f).cuda()
    for hw in (0, 2):
        expect = O.neighbourhood(f, hw, gridpp.Median)
        close(gridpp.neighbourhood(f, hw, gridpp.Median), expect, exact=True)
        close(gridpp.neighbourhood(t, hw, gridpp.Median).cpu().numpy(), expect, exact=True)
