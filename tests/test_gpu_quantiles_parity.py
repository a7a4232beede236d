"""GPU: calc_quantiles and quantile_mapping_curves (gridpp_amd/csrc/rows_quantiles.hip) against the numpy restatement of calc_quantile's
result contract (tests/rows_select_ref.quantile, itself held to the CPU oracle by tests/test_rows_select_restatement.py), per (row, level)
and bit for bit: NaN where it has NaN, identical uint32 views elsewhere, no case exempted.  The three paths (tile, block, loop) are forced
with GPP_ROWS_QUANTILES where their preconditions hold, and the default dispatch runs beside them; a restatement is computed once per
(data, levels) and shared by the paths."""
import contextlib
import functools

import numpy as np
import pytest

from tests import rows_select_ref as ref
from tests.test_gpu_neighbourhood_edges import rows

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")
BLOCK_MAXLEN = 8192                                  # RQ_BLOCK_MAXLEN of rows_quantiles.hip: the longest row the block path sorts
TILE_LENGTHS = [1, 2, 3, 31, 32, 33, 50, 63, 64, 65, 127, 128, 129, 159, 160]      # each side of every power of two the network pads to
BLOCK_LENGTHS = [161, 255, 256, 257, 1000, 1024, 1025, 2048, 2049, 3584, 3585, 4095, 4096, 4097, BLOCK_MAXLEN - 1, BLOCK_MAXLEN, BLOCK_MAXLEN + 1]
TILE_ROW_COUNTS = [1, 63, 64, 65, 129]              # full tiles of 64 rows, a partial last tile, a single row
BLOCK_ROW_COUNTS = [1, 2, 3, 4, 5]
LEVELS = {
    "one": [0.3],                                                       # nq == 1: the loop path whatever is forced
    "two": [0.9, 0.1],                                                  # unsorted
    "ends": [0.5, 0.0, NAN, 1.0, 0.25],                                 # 0, 1 and NaN mixed with interior levels
    "repeated": [0.75, 0.25, 0.75, 0.5, 0.5, 0.1],                      # unsorted and repeated
    "exact": [0.125, 0.875, 0.25, 0.75, 0.5, 0.0625],                   # q (N - 1) is an exact integer on the full rows of 33, 65, 129, 257, 4097 ...
    # The default dispatch sorts from 2 levels on for rows of up to 128 values and of 161 ... 2048, from 3 for 129 ... 160 and 2049 ... 3584, from 4 for 3585 ... 4096 and
    # from 5 beyond: "one" ... "interior4" and the 5 levels of "ends" lie on each side of every one of these gates
    "interior3": [0.2, 0.5, 0.8], "interior4": [0.2, 0.4, 0.6, 0.8],
    "many": [float(x) for x in np.linspace(0, 1, 101, dtype=F)],        # 101 levels: seven chunks of results per tile, the last one partial
    "seventeen": [float(x) for x in np.linspace(0.01, 0.99, 17, dtype=F)],   # one full chunk of 16 and a chunk of one
}
EVERY = ["one", "two", "ends", "repeated", "exact", "interior3", "interior4"]


@pytest.fixture(scope="module")
def api():
    import torch
    import gridpp_amd as gridpp
    return gridpp, torch


@contextlib.contextmanager
def forced(gridpp, path):
    if path is not None:
        assert path in ("tile", "block", "loop")                      # the values rows_quantiles.hip knows
        gridpp.set_path_override("GPP_ROWS_QUANTILES", path)
        assert "GPP_ROWS_QUANTILES" in gridpp.active_overrides()     # the library holds the override under this name
    try:
        yield
    finally:
        gridpp.set_path_override("GPP_ROWS_QUANTILES", None)
        assert "GPP_ROWS_QUANTILES" not in gridpp.active_overrides()


def special(L):
    """all NaN, one valid value, +-inf among finite values, heavy duplicates, and the two smallest rows on which a sorted row answers
    Min / Max wrongly (padded with NaN): [+0.0, -0.0] and [-0.0, +0.0, NaN]"""
    i = np.arange(L)
    out = [np.full(L, np.nan, F), np.where(i == L - 1, F(-4.5), F(np.nan)).astype(F),
           np.where(i % 5 == 0, np.inf, np.where(i % 7 == 0, -np.inf, i * 0.5 - 3)).astype(F), (i % 3).astype(F)]
    for zeros in ([0.0, -0.0], [-0.0, 0.0, np.nan]):
        if L >= len(zeros):
            z = np.full(L, np.nan, F)
            z[:len(zeros)] = zeros
            out.append(z)
            out.append(z[::-1].copy())
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def tile_data(L):
    """129 rows: the rows of the neighbourhood tests, rows_select_ref.adversarial and the special rows first"""
    b = np.concatenate([special(L), ref.adversarial(L), rows(L)])
    a = np.ascontiguousarray(b[np.arange(129) % b.shape[0]])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def block_data(L):
    """5 rows: mixed invalid values, +-0.0 and +-1 only, [-0.0, +0.0, NaN ...], a full row (no invalid value), the zeros of adversarial"""
    adv, r = ref.adversarial(L), rows(L)
    a = np.ascontiguousarray(np.stack([r[0], r[4], special(L)[6], adv[8], adv[1]]))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def adversarial_data(L):
    a = np.concatenate([special(L), ref.adversarial(L)])
    a.setflags(write=False)
    return a


DATA = {"tile": tile_data, "block": block_data, "adversarial": adversarial_data}


@functools.lru_cache(maxsize=None)
def want(kind, L, levels):
    """the restatement per (row, level), computed once and shared by the paths"""
    w = np.array([[ref.quantile(r, q) for q in LEVELS[levels]] for r in DATA[kind](L)], F)
    w.setflags(write=False)
    return w


def device(a):
    """a fresh device tensor with the values of a (possibly read-only) host array"""
    import torch
    return torch.from_numpy(np.array(a, F)).cuda()


def identical(got, expect):
    got, expect = np.asarray(got), np.asarray(expect, F)
    assert got.dtype == F and got.shape == expect.shape, (got.dtype, got.shape, expect.shape)
    ng, ne = np.isnan(got), np.isnan(expect)
    assert (ng == ne).all(), np.argwhere(ng != ne)[:5]
    diff = (got.view(np.uint32) != expect.view(np.uint32)) & ~ng
    assert not diff.any(), (np.argwhere(diff)[:5], got[diff][:5], expect[diff][:5])


def check(api, kind, L, counts, names):
    gridpp, torch = api
    a = DATA[kind](L)
    t = device(a)
    for name in names:
        w = want(kind, L, name)
        for R in counts:
            identical(gridpp.calc_quantiles(t[:R], LEVELS[name]).cpu().numpy(), w[:R])


# ---- paths and lengths --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", TILE_LENGTHS)
@pytest.mark.parametrize("path", [None, "tile", "loop"])
def test_short_rows(api, path, L):
    """rows of up to 160 values on every row count and level set, through one path (None: the default dispatch)"""
    with forced(api[0], path):
        check(api, "tile", L, TILE_ROW_COUNTS, EVERY)


@pytest.mark.parametrize("L", BLOCK_LENGTHS)
@pytest.mark.parametrize("path", [None, "block", "loop"])
def test_long_rows(api, path, L):
    """rows beyond the tile limit, up to one past the longest the block path sorts (which the loop path takes whatever is forced)"""
    with forced(api[0], path):
        check(api, "block", L, BLOCK_ROW_COUNTS, EVERY)


@pytest.mark.parametrize("L", [161, 1000, 4097])
@pytest.mark.parametrize("path", [None, "block", "loop"])
def test_long_adversarial_rows(api, path, L):
    with forced(api[0], path):
        check(api, "adversarial", L, [17], ["ends", "repeated", "exact"])


@pytest.mark.parametrize("kind,L", [("tile", 33), ("tile", 50), ("tile", 160), ("adversarial", 257), ("adversarial", 1000)])
@pytest.mark.parametrize("path", [None, "tile", "block", "loop"])
def test_many_levels(api, path, kind, L):
    """101 levels (0 and 1 among them) and 17: the chunks of staged results of the tile path, more levels than a wave has lanes on block"""
    counts = [129, 65] if kind == "tile" else [17]
    with forced(api[0], path):
        check(api, kind, L, counts, ["many", "seventeen"])


@functools.lru_cache(maxsize=None)
def beyond():
    """2 rows of 70 001 values, their levels and the restatement"""
    rng = np.random.default_rng(7)
    a = rng.normal(280, 15, (2, 70001)).astype(F)
    a[:, ::97] = np.nan
    a[1, 5::1001] = np.inf
    a[0, 7] = -0.0
    levels = LEVELS["ends"] + LEVELS["two"]
    return a, levels, np.array([[ref.quantile(r, q) for q in levels] for r in a], F)


@pytest.mark.parametrize("path", [None, "tile", "block", "loop"])
def test_rows_beyond_every_sorting_path(api, path):
    """rows of 70 001 values: the loop path whatever is forced"""
    a, levels, w = beyond()
    with forced(api[0], path):
        identical(api[0].calc_quantiles(device(a), levels).cpu().numpy(), w)


@pytest.mark.parametrize("path", [None, "tile", "loop"])
def test_zeros_of_mixed_sign(api, path):
    """the smallest rows on which a sort answers Min / Max wrongly: the FIRST zero in the original order is both extremes"""
    gridpp, torch = api
    levels = [0.0, 0.5, 1.0]
    with forced(gridpp, path):
        for row in ([0.0, -0.0], [-0.0, 0.0, NAN], [-0.0, 0.0], [NAN, 0.0, -0.0]):
            a = np.array([row] * 3, F)
            got = gridpp.calc_quantiles(device(a), levels).cpu().numpy()
            identical(got, [[ref.quantile(a[0], q) for q in levels]] * 3)
            assert np.signbit(got[0, 0]) == np.signbit(F(row[0] if not np.isnan(row[0]) else row[1])) and np.signbit(got[0, 2]) == np.signbit(got[0, 0])


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 50, 160, 257])
def test_unaligned_input(api, L):
    """a view that starts one float into a buffer gives the bits of the aligned copy"""
    gridpp, torch = api
    kind, R = ("tile", 129) if L <= 160 else ("adversarial", 17)
    a = DATA[kind](L) if L != 4 else tile_data(50)[:, :4]
    buf = torch.empty(R * L + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(R, L)
    view.copy_(device(a[:R]))
    assert view.data_ptr() % 16 == 4
    w = np.array([[ref.quantile(r, q) for q in LEVELS["ends"]] for r in a[:R]], F)
    for path in (None, "tile", "block"):
        with forced(gridpp, path):
            identical(gridpp.calc_quantiles(view, LEVELS["ends"]).cpu().numpy(), w)


@pytest.mark.parametrize("L", [50, 1000])
def test_host_device_cube_and_float64_input_agree(api, L):
    gridpp, torch = api
    kind = "tile" if L <= 160 else "adversarial"
    a = DATA[kind](L)[:12]
    w = want(kind, L, "ends")[:12]
    t = device(np.ascontiguousarray(a))
    dev = gridpp.calc_quantiles(t, LEVELS["ends"])
    assert isinstance(dev, torch.Tensor) and dev.device == t.device and dev.dtype == torch.float32 and tuple(dev.shape) == (12, 5)
    host = gridpp.calc_quantiles(a, LEVELS["ends"])
    assert isinstance(host, np.ndarray) and host.dtype == F and host.shape == (12, 5)
    identical(host, w)
    identical(dev.cpu().numpy(), w)
    identical(gridpp.calc_quantiles(a.astype(np.float64), np.array(LEVELS["ends"], np.float64)), w)      # float64 host input
    identical(gridpp.calc_quantiles(t, torch.tensor(LEVELS["ends"], device="cuda")).cpu().numpy(), w)    # device levels are copied to the host
    cube = gridpp.calc_quantiles(t.reshape(3, 4, L), LEVELS["ends"])                                     # the cube form
    assert isinstance(cube, torch.Tensor) and tuple(cube.shape) == (3, 4, 5) and cube.device == t.device
    identical(cube.cpu().numpy().reshape(12, 5), w)
    identical(gridpp.calc_quantiles(a.reshape(3, 4, L), LEVELS["ends"]), w.reshape(3, 4, 5))
    one = gridpp.calc_quantiles(t[0], LEVELS["ends"])                                                    # the vector form
    assert isinstance(one, torch.Tensor) and tuple(one.shape) == (5,)
    identical(one.cpu().numpy(), w[0])
    identical(gridpp.calc_quantiles(a[0], LEVELS["ends"]), w[0])


@pytest.mark.parametrize("L", [50, 160, 161, 4097])
def test_one_level_is_calc_quantile(api, L):
    """calc_quantiles(a, [q])[:, 0] == calc_quantile(a, q), and so is every column of a call with many levels"""
    gridpp, torch = api
    kind = "tile" if L <= 160 else "block"
    t = device(DATA[kind](L))
    for q in (0.0, 0.3, 0.5, 1.0, NAN):
        identical(gridpp.calc_quantiles(t, [q])[:, 0].cpu().numpy(), gridpp.calc_quantile(t, q).cpu().numpy())
    got = gridpp.calc_quantiles(t, LEVELS["ends"]).cpu().numpy()
    for j, q in enumerate(LEVELS["ends"]):
        identical(got[:, j], gridpp.calc_quantile(t, q).cpu().numpy())


def test_empty_shapes_and_errors_on_tensors(api):
    gridpp, torch = api
    t = device(tile_data(50))
    for shape, q, expect in (((0, 5), [0.5], (0, 1)), ((3, 5), [], (3, 0)), ((2, 0, 5), [0.1, 0.2], (2, 0, 2))):
        out = gridpp.calc_quantiles(torch.empty(shape, device="cuda"), q)
        assert isinstance(out, torch.Tensor) and out.device == t.device and tuple(out.shape) == expect
    out = gridpp.calc_quantiles(torch.empty((3, 0), device="cuda"), [0.5, 0.0])          # rows without a value
    assert tuple(out.shape) == (3, 2) and bool(torch.isnan(out).all())
    with pytest.raises(ValueError, match="calc_quantiles: Quantiles must be between 0 and 1 inclusive"):
        gridpp.calc_quantiles(t, [0.5, 1.0001])
    with pytest.raises(RuntimeError, match="array must have 1, 2 or 3 dimensions"):
        gridpp.calc_quantiles(torch.empty((2, 2, 2, 2), device="cuda"), [0.5])
    with pytest.raises(ValueError, match="either all field arguments"):
        gridpp.quantile_mapping_curves(t.reshape(3, 43, 50), tile_data(50).reshape(3, 43, 50), [0.5])


# ---- quantile_mapping_curves ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cubes():
    rng = np.random.default_rng(11)
    r, f = rng.normal(5, 2, (5, 7, 40)).astype(F), rng.gamma(2, 2, (5, 7, 33)).astype(F)
    r[rng.random(r.shape) < 0.05] = np.nan
    f[rng.random(f.shape) < 0.05] = np.nan
    r[1, 2], f[1, 2] = np.nan, np.nan              # a cell of all-NaN
    r[3, 4], f[3, 4] = np.nan, np.nan              # a cell with one valid value
    r[3, 4, 0], f[3, 4, -1] = 2.5, 7.0
    levels = [float(x) for x in np.linspace(0, 1, 11, dtype=F)]
    cr = np.array([[[ref.quantile(c, q) for q in levels] for c in plane] for plane in r], F)
    cf = np.array([[[ref.quantile(c, q) for q in levels] for c in plane] for plane in f], F)
    for x in (r, f, cr, cf):
        x.setflags(write=False)
    return r, f, levels, cr, cf


@pytest.mark.parametrize("path", [None, "tile", "loop"])
def test_quantile_mapping_curves_per_cell(api, path):
    gridpp, torch = api
    r, f, levels, cr, cf = cubes()
    with forced(gridpp, path):
        host = gridpp.quantile_mapping_curves(r, f, levels)
        dev = gridpp.quantile_mapping_curves(device(r), device(f), levels)
    for got, expect in zip(host, (cr, cf)):
        assert isinstance(got, np.ndarray) and got.shape == (5, 7, 11)
        identical(got, expect)
    for got, expect in zip(dev, (cr, cf)):
        assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (5, 7, 11)
        identical(got.cpu().numpy(), expect)
    assert np.isnan(host[0][1, 2]).all() and (host[0][3, 4] == r[3, 4, 0]).all()


def test_curves_feed_apply_curve_on_the_device(api):
    """apply_curve with the curves this function returned == the same call with curves built per cell on the host from the restatement"""
    gridpp, torch = api
    r, f, levels, cr, cf = cubes()
    field = torch.from_numpy(np.random.default_rng(12).gamma(2, 2.5, (5, 7)).astype(F)).cuda()
    curve_ref, curve_fcst = gridpp.quantile_mapping_curves(device(r), device(f), levels)
    got = gridpp.apply_curve(field, curve_ref, curve_fcst, gridpp.OneToOne, gridpp.MeanSlope)
    expect = gridpp.apply_curve(field, device(cr), device(cf), gridpp.OneToOne, gridpp.MeanSlope)
    assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (5, 7)
    identical(got.cpu().numpy(), expect.cpu().numpy())
    assert int(torch.isfinite(got).sum()) >= 33          # (every cell but the all-NaN one, and the one-valid one at most, maps to a number)
