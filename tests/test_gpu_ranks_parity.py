"""GPU: calc_ranks, sort_rows, reorder_by_ranks and calc_crps (gridpp_amd/csrc/rows_rank.hip) against the numpy restatement
tests/rows_rank_ref.py (held to the counting definition by tests/test_ranks_api.py).  Ranks are compared as integers; sorted and reordered
rows bit for bit (NaN positions first, then the uint32 views); the CRPS per row with the float32 cast of the restatement's float64 PAIRWISE
value, within one float32 ulp of that value plus 8 N 2^-53 (max |x| + |y|) computed from the row -- the double sums differ from the
restatement's only in their order of summation, by that term, and the final cast moves the result by at most one ulp when the two doubles
fall on either side of a rounding boundary.  No case is exempted.  The three paths (tile, block, long) are forced with GPP_ROWS_RANKS where
their preconditions hold and the default dispatch runs beside them; a restatement is computed once per length and shared by the paths."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

from tests import rows_rank_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
TILE_LENGTHS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 50, 63, 64, 65, 127, 128, 129, 159, 160]   # each side of every sweep of eight and power of two
TILE_ROW_COUNTS = [1, 63, 64, 65, 129]               # a single row, a partial tile, a full one, several tiles with a partial last one
BLOCK_LENGTHS = [161, 255, 256, 257, 1000, 1024, 1025, 4097, 8192]
BLOCK_ROW_COUNTS = [1, 2, 3, 4, 5]
LONG_CASES = [(8193, 3), (70001, 2)]
PATTERNS = 12


@pytest.fixture(scope="module")
def api():
    import torch
    import gridpp_amd as gridpp
    return gridpp, torch


@contextlib.contextmanager
def forced(gridpp, path):
    if path is not None:
        assert path in ("tile", "block", "long")                     # the values rows_rank.hip knows
        gridpp.set_path_override("GPP_ROWS_RANKS", path)
        assert "GPP_ROWS_RANKS" in gridpp.active_overrides()         # the library holds the override under this name
    try:
        yield
    finally:
        gridpp.set_path_override("GPP_ROWS_RANKS", None)
        assert "GPP_ROWS_RANKS" not in gridpp.active_overrides()


def pattern_row(p, L, rng, sparse):
    """one row of every kind the issue names; `sparse`: the fraction of NaN of the random kinds"""
    i = np.arange(L)
    if p == 0:
        row = rng.normal(0, 1, L)
    elif p == 1:
        return np.full(L, np.nan, F)                                                      # all NaN
    elif p == 2:
        return np.where(i == L - 1, F(-4.5), F(np.nan)).astype(F)                         # one valid value
    elif p == 3:
        return np.where(i % 5 == 0, np.inf, np.where(i % 7 == 0, -np.inf, i * 0.5 - 3)).astype(F)   # +-inf among finite values
    elif p == 4:
        return (i % 3).astype(F)                                                          # heavy duplicates
    elif p == 5:
        return np.full(L, 2.5, F)                                                         # all equal
    elif p == 6:
        return np.where(i % 2 == 0, F(-0.0), F(0.0)).astype(F)                            # tied zeros, -0.0 and +0.0 interleaved
    elif p == 7:
        return (i * 0.25 - 7).astype(F)                                                   # already sorted
    elif p == 8:
        return (7 - i * 0.25).astype(F)                                                   # reversed
    elif p == 9:
        row = rng.normal(0, 1e-3, L)
        sparse = max(sparse, 0.5)
    elif p == 10:
        row = rng.integers(-1, 2, L).astype(np.float64)                                   # -1, +-0.0, 1 and NaN
        row[(row == 0) & (rng.random(L) < 0.5)] = -0.0
    else:
        row = np.maximum(rng.gamma(0.5, 2, L) - 1, 0) * 1e5                               # many tied zeros under a long tail
    row = row.astype(F)
    row[rng.random(L) < sparse] = np.nan
    return row


@functools.lru_cache(maxsize=None)
def data(L, R, shift=0, sparse=0.1):
    """R rows of length L; row n is of kind (n + shift) % 12; read-only"""
    rng = np.random.default_rng(1000 * L + shift)
    a = np.stack([pattern_row((n + shift) % PATTERNS, L, rng, sparse) for n in range(R)])
    a.setflags(write=False)
    return a


def refs_for(a, seed):
    """one y per row: equal to every member of an all-equal row (a CRPS of exactly 0), else a value near the ensemble, NaN, one far outside, inf"""
    rng = np.random.default_rng(seed)
    y = np.array([[rng.normal(), np.nan, 1e6, np.inf, -0.3][n % 5] for n in range(a.shape[0])], F)
    for n, row in enumerate(a):
        v = row[np.isfinite(row)]
        if v.size and (v == v[0]).all() and n % 2 == 0:
            y[n] = v[0]
    return y


class Want:
    """the restatement of every function on one (values, template, ref) triple, computed once"""

    def __init__(self, a, t):
        self.a, self.t, self.y = a, t, refs_for(a, a.shape[1])
        self.ranks = ref.rows_of(ref.ranks, a).astype(np.int32)
        self.sorted = ref.rows_of(ref.sorted_row, a).astype(F)
        self.reorder = ref.rows_of(ref.reorder, a, t).astype(F)
        self.crps = ref.crps(a, self.y)
        self.slack = np.array([ref.crps_slack(r, y) for r, y in zip(a, self.y)])


def shift_of(L, lengths):
    return 5 * lengths.index(L) if L in lengths else 0


@functools.lru_cache(maxsize=None)
def want(L, R, lengths=None, sparse=0.1):
    s = shift_of(L, lengths) if lengths else 0
    return Want(data(L, R, s, sparse), data(L, R, s + 3, sparse))


def device(a):
    """a fresh device tensor with the values of a (possibly read-only) host array"""
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def identical(got, expect):
    got, expect = np.asarray(got), np.asarray(expect, F)
    assert got.dtype == F and got.shape == expect.shape, (got.dtype, got.shape, expect.shape)
    ng, ne = np.isnan(got), np.isnan(expect)
    assert (ng == ne).all(), np.argwhere(ng != ne)[:5]
    diff = (got.view(np.uint32) != expect.view(np.uint32)) & ~ng
    assert not diff.any(), (np.argwhere(diff)[:5], got[diff][:5], expect[diff][:5])


def same_ranks(got, expect):
    got = np.asarray(got)
    assert got.dtype == np.int32 and got.shape == expect.shape, (got.dtype, got.shape)
    bad = got != expect
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], expect[bad][:5])


def crps_close(got, want64, slack):
    got = np.asarray(got)
    assert got.dtype == F and got.shape == want64.shape, (got.dtype, got.shape)
    w32 = want64.astype(F)
    ng, nw = np.isnan(got), np.isnan(w32)
    assert (ng == nw).all(), np.argwhere(ng != nw)[:5]
    ok = ~nw
    err = np.abs(got[ok].astype(np.float64) - w32[ok].astype(np.float64))
    bound = np.spacing(np.abs(w32[ok])).astype(np.float64) + slack[ok]
    assert (err <= bound).all(), (np.argwhere(err > bound)[:5], got[ok][err > bound][:5], w32[ok][err > bound][:5])


def check_all(gridpp, w, R, a_dev=None, t_dev=None, y_dev=None):
    """the four functions on the first R rows of a Want, on device tensors"""
    a = device(w.a[:R]) if a_dev is None else a_dev
    t = device(w.t[:R]) if t_dev is None else t_dev
    y = device(w.y[:R]) if y_dev is None else y_dev
    ranks, srt = gridpp.calc_ranks(a), gridpp.sort_rows(a)
    same_ranks(ranks.cpu().numpy(), w.ranks[:R])
    identical(srt.cpu().numpy(), w.sorted[:R])
    got = gridpp.reorder_by_ranks(a, t)
    identical(got.cpu().numpy(), w.reorder[:R])
    crps_close(gridpp.calc_crps(a, y).cpu().numpy(), w.crps[:R], w.slack[:R])
    return ranks, srt, got


def composition(torch, gridpp, a, t, got):
    """reorder_by_ranks == sort_rows(values) gathered by calc_ranks(template), NaN for a rank of -1 or beyond the valid values, bit for bit"""
    s, r = gridpp.sort_rows(a), gridpp.calc_ranks(t).long()
    nv = torch.isfinite(a).sum(-1, keepdim=True)
    comp = torch.where((r >= 0) & (r < nv), torch.gather(s, -1, r.clamp(min=0)), torch.full_like(s, float("nan")))
    identical(got.cpu().numpy(), comp.cpu().numpy())


# ---- the paths ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["tile", None])
def test_tile_lengths_and_row_counts(api, path):
    gridpp, torch = api
    with forced(gridpp, path):
        for L in TILE_LENGTHS:
            w = want(L, 129)
            for R in TILE_ROW_COUNTS:
                a, t = device(w.a[:R]), device(w.t[:R])
                ranks, srt, got = check_all(gridpp, w, R, a, t)
                if R == 129:
                    composition(torch, gridpp, a, t, got)
                    # sort_rows(a)[rank] == a bit for bit on every valid element (position decides among the tied zeros of either sign)
                    ok = ranks >= 0
                    back = torch.gather(srt, -1, ranks.long().clamp(min=0))
                    assert torch.equal(back.view(torch.int32)[ok], a.view(torch.int32)[ok]), L


def test_tile_unaligned_view(api):
    """a view that starts 4 bytes behind a 16-byte boundary takes the 4-byte staging"""
    gridpp, torch = api
    for L in (7, 50, 160):
        w = want(L, 129)
        views = []
        for src in (w.a, w.t):
            base = torch.empty(129 * L + 1, dtype=torch.float32, device="cuda")
            base[1:] = device(src).reshape(-1)
            views.append(base[1:].reshape(129, L))
            assert views[-1].data_ptr() % 16 == 4 and views[-1].is_contiguous()
        check_all(gridpp, w, 129, views[0], views[1])


@pytest.mark.parametrize("path", ["block", None])
def test_block_lengths_and_row_counts(api, path):
    gridpp, torch = api
    with forced(gridpp, path):
        for L in BLOCK_LENGTHS:
            w = want(L, 5, tuple(BLOCK_LENGTHS))
            for R in (BLOCK_ROW_COUNTS if L <= 1025 else [5]):
                a, t = device(w.a[:R]), device(w.t[:R])
                got = check_all(gridpp, w, R, a, t)[2]
            composition(torch, gridpp, a, t, got)


def test_long_path(api):
    """rows beyond the block path by default, and the long path forced on tile and block lengths"""
    gridpp, torch = api
    for L, R in LONG_CASES:
        w = want(L, R, None, 0.5 if L < 10000 else 0.97)          # (the pairwise restatement is O(N^2): the long rows are mostly NaN)
        a, t = device(w.a), device(w.t)
        composition(torch, gridpp, a, t, check_all(gridpp, w, R, a, t)[2])
        dense = data(L, R, 5, 0.1)                                # ranks and sorted rows of long rows that are mostly valid
        d = device(dense)
        same_ranks(gridpp.calc_ranks(d).cpu().numpy(), ref.rows_of(ref.ranks, dense).astype(np.int32))
        identical(gridpp.sort_rows(d).cpu().numpy(), ref.rows_of(ref.sorted_row, dense))
    with forced(gridpp, "long"):
        for L, R in ((1, 3), (7, 129), (50, 65), (160, 64)):
            check_all(gridpp, want(L, 129), R)
        for L in (161, 1025):
            check_all(gridpp, want(L, 5, tuple(BLOCK_LENGTHS)), 5)


def test_forcing_a_path_where_it_does_not_apply_changes_nothing(api):
    gridpp, torch = api
    with forced(gridpp, "block"):
        check_all(gridpp, want(50, 129), 65)
    with forced(gridpp, "tile"):
        check_all(gridpp, want(161, 5, tuple(BLOCK_LENGTHS)), 5)


# ---- data the kinds above do not pin by themselves ----------------------------------------------------------------------------------------------
def test_known_answers(api):
    gridpp, torch = api
    nan, inf = np.nan, np.inf
    a = np.array([[3, 1, nan, 1, inf, 0.0, -0.0], [-0.0, 0.0, -0.0, 0.0, nan, nan, nan]], F)
    assert gridpp.calc_ranks(a).tolist() == [[4, 2, -1, 3, -1, 0, 1], [0, 1, 2, 3, -1, -1, -1]]
    s = gridpp.sort_rows(a)
    identical(s, np.array([[0.0, -0.0, 1, 1, 3, nan, nan], [-0.0, 0.0, -0.0, 0.0, nan, nan, nan]], F))
    v, t = np.array([10, nan, 30, 20], F), np.array([0.5, 0.1, 0.9, 0.7], F)
    identical(gridpp.reorder_by_ranks(v, t), np.array([20, 10, nan, 30], F))        # the template's rank 3 is not below the 3 valid values
    identical(gridpp.reorder_by_ranks(t, v), np.array([0.1, nan, 0.7, 0.5], F))     # an invalid template value
    e = np.array([[1, 2, 3, nan], [5, nan, nan, nan], [2, 2, 2, 2], [nan, inf, nan, -inf], [1, 2, 3, 4], [1, 2, 3, 4], [0, 1, 0, 1]], F)
    y = np.array([2, 7, 2, 0, nan, -inf, 1e6], F)
    got = gridpp.calc_crps(e, y)
    assert got[1] == 2.0 and got[2] == 0.0 and np.isnan(got[[3, 4, 5]]).all()       # N = 1 is |x - y|; y equal to every member is exactly 0
    crps_close(got, ref.crps(e, y), np.array([ref.crps_slack(r, v) for r, v in zip(e, y)]))
    assert abs(float(got[0]) - (2 / 3 - 4 / 9)) < 1e-7 and abs(float(got[6]) - (1e6 - 0.5 - 0.25)) < 0.0625


# ---- interfaces ---------------------------------------------------------------------------------------------------------------------------
def test_host_device_shapes_and_float64(api):
    gridpp, torch = api
    L = 50
    w = want(L, 129)
    a, t, y = np.array(w.a[:12]), np.array(w.t[:12]), np.array(w.y[:12])
    for conv in (lambda x: x, lambda x: x.astype(np.float64)):                           # host arrays, float32 and float64
        r, s, o, c = gridpp.calc_ranks(conv(a)), gridpp.sort_rows(conv(a)), gridpp.reorder_by_ranks(conv(a), conv(t)), gridpp.calc_crps(conv(a), conv(y))
        assert all(isinstance(x, np.ndarray) for x in (r, s, o, c))
        same_ranks(r, w.ranks[:12]); identical(s, w.sorted[:12]); identical(o, w.reorder[:12]); crps_close(c, w.crps[:12], w.slack[:12])
    da, dt, dy = device(a), device(t), device(y)
    cube = lambda x: x.reshape((3, 4) + tuple(x.shape[1:]))                              # the cube form, on both sides
    for A, T, Y in ((cube(da), cube(dt), cube(dy)), (cube(a), cube(t), cube(y))):
        r, s, o, c = gridpp.calc_ranks(A), gridpp.sort_rows(A), gridpp.reorder_by_ranks(A, T), gridpp.calc_crps(A, Y)
        dev = hasattr(A, "is_cuda")
        assert all((getattr(x, "is_cuda", False)) == dev for x in (r, s, o, c))
        host = (lambda x: x.cpu().numpy()) if dev else (lambda x: x)
        assert tuple(r.shape) == (3, 4, L) and tuple(c.shape) == (3, 4)
        same_ranks(host(r), cube(w.ranks[:12])); identical(host(s), cube(w.sorted[:12])); identical(host(o), cube(w.reorder[:12]))
        crps_close(host(c), cube(w.crps[:12]), cube(w.slack[:12]))
    for n in (0, 4, 6):                                                                  # the vector form
        same_ranks(gridpp.calc_ranks(da[n]).cpu().numpy(), w.ranks[n]); identical(gridpp.sort_rows(a[n]), w.sorted[n])
        identical(gridpp.reorder_by_ranks(da[n], dt[n]).cpu().numpy(), w.reorder[n])
        c = gridpp.calc_crps(da[n], dy[n])
        assert tuple(c.shape) == ()
        crps_close(c.cpu().numpy().reshape(1), w.crps[n:n + 1], w.slack[n:n + 1])
    assert torch.isnan(gridpp.calc_crps(torch.empty((3, 0), device="cuda"), torch.zeros(3, device="cuda"))).all()   # rows without a member
    assert gridpp.calc_ranks(torch.empty((0, 5), device="cuda")).dtype == torch.int32


def test_c_abi_either_output_null(api):
    """gpp_calc_ranks writes the outputs it is given -- both from one launch -- and leaves nothing else behind"""
    gridpp, torch = api
    from gridpp_amd import _capi
    lib = _capi.lib()
    for L, R, lengths in ((50, 129, None), (160, 65, None), (257, 5, tuple(BLOCK_LENGTHS))):
        w = want(L, 129 if lengths is None else 5, lengths)
        a = device(w.a[:R])
        p = lambda x: C.c_void_p(x.data_ptr())
        for want_ranks, want_sorted in ((1, 1), (1, 0), (0, 1)):
            ranks = torch.full((R, L), -7, dtype=torch.int32, device="cuda")
            srt = torch.full((R, L), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert lib.gpp_calc_ranks(p(a), R, L, p(ranks) if want_ranks else None, p(srt) if want_sorted else None, _capi.MEM_DEVICE) == _capi.GPP_OK
            if want_ranks:
                same_ranks(ranks.cpu().numpy(), w.ranks[:R])
            else:
                assert (ranks == -7).all()
            if want_sorted:
                identical(srt.cpu().numpy(), w.sorted[:R])
            else:
                assert (srt == -7).all()
    host_ranks, host_sorted = np.full((12, 50), -7, np.int32), np.full((12, 50), -7, F)  # the host path stages the int32 output too
    w = want(50, 129)
    h = np.array(w.a[:12])
    assert lib.gpp_calc_ranks(C.c_void_p(h.ctypes.data), 12, 50, C.c_void_p(host_ranks.ctypes.data), C.c_void_p(host_sorted.ctypes.data), _capi.MEM_HOST) == _capi.GPP_OK
    same_ranks(host_ranks, w.ranks[:12]); identical(host_sorted, w.sorted[:12])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def test_calibrated_quantiles_get_their_members_back(api):
    """raw cube -> calc_quantiles at the E levels (i + 1) / (E + 1) -> reorder_by_ranks(quantiles, raw), all on device tensors: every cell
    holds the multiset of its quantiles in the rank order of the raw cell, and the CRPS does not care about the order"""
    gridpp, torch = api
    Y, X, E = 9, 11, 50
    rng = np.random.default_rng(418)
    raw = device(rng.gamma(2, 2, (Y, X, E)).astype(F))
    obs = device(rng.gamma(2, 2, (Y, X)).astype(F))
    levels = [(i + 1) / (E + 1) for i in range(E)]
    q = gridpp.calc_quantiles(raw, levels)
    out = gridpp.reorder_by_ranks(q, raw)
    assert out.shape == raw.shape and out.is_cuda
    identical(gridpp.sort_rows(out).cpu().numpy(), gridpp.sort_rows(q).cpu().numpy())
    assert torch.equal(gridpp.calc_ranks(out), gridpp.calc_ranks(raw))
    a, b = gridpp.calc_crps(out, obs).cpu().numpy(), gridpp.calc_crps(q, obs).cpu().numpy()
    qh, oh = q.cpu().numpy().reshape(-1, E), obs.cpu().numpy().reshape(-1)
    slack = np.array([ref.crps_slack(r, y) for r, y in zip(qh, oh)]).reshape(Y, X)
    assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)) + slack).all()
    crps_close(b, ref.crps(qh, oh).reshape(Y, X), slack)
