"""Neighbourhood paths on both sides of the limits at which the host code changes kernels, against the CPU oracle (through the C-ABI).

gridpp_amd/csrc/neighbourhood.hip picks a path from the member count E (rows of up to MEMBER_EC = 160 members go through LDS, byte
counts hold up to 254), the number of thresholds (the fused quantile_fast path takes up to 16), the halfwidth (fused box passes up
to 16), the alignment of a device pointer and what the previous call left behind (the speculative count pass, the padding of the
count planes).  The tests here cross each of those limits."""
import contextlib

import numpy as np
import pytest

from tests.test_gpu_neighbourhood_parity import RTOL, close, field

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24      # unit roundoff of float32


@pytest.fixture(scope="module")
def api():
    import gridpp_amd as gridpp
    from oracle import oracle as O
    return gridpp, O


@contextlib.contextmanager
def override(gridpp, *names):
    for n in names:
        gridpp.set_path_override(n, "1")
    try:
        yield
    finally:
        for n in names:
            gridpp.set_path_override(n, None)


def members(seed, Y, X, E, invalid=True, integer=False, spread=True):
    """(Y, X, E) members.  spread: offset and scale vary from cell to cell (the per-cell Std / Variance planes then vary across the
    field, so the box Std / Variance of them does not cancel).  invalid: NaN, +inf and -inf members, cells with none valid."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0, 10, (Y, X, E))
    if integer:
        f = np.floor(f)
    if spread:
        f = f * rng.uniform(0.1, 3, (Y, X, 1)) + rng.uniform(-20, 20, (Y, X, 1))
    f = f.astype(np.float32)
    if invalid:
        r = rng.random(f.shape)
        f[r < 0.03] = np.nan
        f[(r >= 0.03) & (r < 0.04)] = np.inf
        f[(r >= 0.04) & (r < 0.05)] = -np.inf
        f[2:4, 3:6, :] = np.nan
        f[Y - 1, X - 1, :] = np.inf
        f[5, 1, :] = -np.inf
    return f


def per_cell(O, f, stat):
    """the plane the 2-D filter of a 3-D call runs on: the oracle's calc_statistic over each cell's members (neighbourhood.cpp:12-27)"""
    Y, X, E = f.shape
    return np.array([O.calc_statistic(f[y, x], stat) for y in range(Y) for x in range(X)], np.float32).reshape(Y, X)


def close_spread(gridpp, O, out, plane, hw, stat):
    """Std / Variance of a 2-D `plane` with the measure of test_gpu_neighbourhood_parity.test_2d_statistics: 1e-5 relative where
    E[x^2] - E[x]^2 does not cancel (variance >= 5 % of E[x^2]); where it does, Variance within 1e-5 of E[x^2] (+ the absolute noise of
    the reference's summed-area table) and Std only NaN-ness and order of magnitude.  Windows without a valid value are NaN."""
    ref = O.neighbourhood(plane, hw, stat)
    m2 = O.neighbourhood(np.where(np.isnan(plane), np.nan, plane * plane).astype(np.float32), hw, gridpp.Mean)
    var_ref = O.neighbourhood(plane, hw, gridpp.Variance)
    empty = np.isnan(O.neighbourhood(plane, hw, gridpp.Mean))
    assert np.isnan(out[empty]).all() and np.isnan(ref[empty]).all()
    cancelling = ~empty & ~(var_ref >= 0.05 * m2)
    plain = ~empty & ~cancelling
    assert not np.isnan(out[plain]).any()
    rel = np.abs(out[plain].astype(np.float64) - ref[plain]) / np.maximum(np.abs(ref[plain]), 1e-30)
    assert (rel < RTOL).all(), rel.max()
    assert plain.sum() > 0.5 * (~empty).sum() or hw == 0      # the tight bound covers most of the field
    if stat == gridpp.Variance:
        assert (np.abs(out[cancelling].astype(np.float64) - ref[cancelling]) <= 1e-5 * m2[cancelling] + 1e-9).all()


def same(a, b):
    """test_quantile_fast_threshold_lists' comparison: infinities agree exactly, the rest to 1e-5"""
    a, b = np.asarray(a), np.asarray(b)
    assert (np.isinf(a) == np.isinf(b)).all() and (a[np.isinf(b)] == b[np.isinf(b)]).all()
    close(np.where(np.isinf(b), np.float32(0), a), np.where(np.isinf(b), np.float32(0), b))


def identical(a, b):
    """bit for bit (NaN where the other is NaN)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32
    na, nb = np.isnan(a), np.isnan(b)
    assert (na == nb).all(), (na != nb).sum()
    diff = (a.view(np.uint32) != b.view(np.uint32)) & ~na
    assert not diff.any(), (int(diff.sum()), a[diff][:4], b[diff][:4])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. 3-D statistics across the LDS row limit (MEMBER_EC = 160: above it the member pass walks each row from memory)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [159, 160, 161, 164, 200, 256])
def test_3d_statistics_across_the_lds_row_limit(api, E):
    """Every statistic of the 3-D form at member counts on both sides of MEMBER_EC, on a field of 43 x 45 cells (the last tile of 64
    cells holds 15), with NaN / +inf / -inf members and cells without a valid member.  The member statistic is the reference's
    sequential float loop on either side of the limit: Count / Min / Max / Median are exact, Mean / Sum within 1e-5, Std / Variance
    within the measure of the 2-D parity test (on the plane of per-cell values)."""
    gridpp, O = api
    Y, X = 43, 45
    f = members(100 + E, Y, X, E)
    for hw in (0, 3, 17):
        for stat in (gridpp.Count, gridpp.Min, gridpp.Max, gridpp.Median):
            close(gridpp.neighbourhood(f, hw, stat), O.neighbourhood(f, hw, stat), exact=True)
        for stat in (gridpp.Mean, gridpp.Sum):
            close(gridpp.neighbourhood(f, hw, stat), O.neighbourhood(f, hw, stat))
        for stat in (gridpp.Std, gridpp.Variance):
            close_spread(gridpp, O, gridpp.neighbourhood(f, hw, stat), per_cell(O, f, stat), hw, stat)


def test_3d_exact_quantile_and_brute_force_at_200_members(api):
    """neighbourhood_quantile and neighbourhood_brute_force gather window x members (here up to 25 x 200 values per cell): exact."""
    gridpp, O = api
    f = members(7, 12, 14, 200, spread=False)
    for q in (0.0, 0.3, 0.5, 1.0):
        close(gridpp.neighbourhood_quantile(f, q, 2), O.neighbourhood_quantile(f, q, 2), exact=True)
    for stat in (gridpp.Mean, gridpp.Median):
        close(gridpp.neighbourhood_brute_force(f, 2, stat), O.neighbourhood_brute_force(f, 2, stat), exact=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. device fields that are not 16-byte aligned (generic member pass, compare-per-threshold count pass)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [None, 8, 20, 100])
def test_misaligned_device_fields(api, E):
    """torch views 1, 2 and 3 floats into a larger allocation: the member pass leaves the LDS-DMA path and quantile_fast the ranked
    count pass (both need 16-byte aligned rows).  Every result is bit for bit the host-array call's (an aligned staging copy) and
    within the usual measure of the oracle."""
    import torch
    gridpp, O = api
    Y, X = 37, 45                     # (1665 cells: a partial last tile)
    f = field(40 + (E or 0), Y, X) if E is None else members(40 + E, Y, X, E)
    thr = np.linspace(-10, 30, 9).astype(np.float32) if E else np.linspace(0, 10, 9).astype(np.float32)
    qf = np.random.default_rng(5).random((Y, X)).astype(np.float32)
    qf[0, 0], qf[1, 1], qf[2, 2] = 0.0, 1.0, np.nan
    stats = (gridpp.Mean, gridpp.Sum, gridpp.Count, gridpp.Min, gridpp.Max, gridpp.Std, gridpp.Variance, gridpp.Median)
    host = {s: gridpp.neighbourhood(f, 3, s) for s in stats}
    hq = (gridpp.neighbourhood_quantile_fast(f, 0.5, 4, thr), gridpp.neighbourhood_quantile_fast(f, qf, 2, thr))
    for s in stats:
        if s in (gridpp.Std, gridpp.Variance):
            close_spread(gridpp, O, host[s], f if E is None else per_cell(O, f, s), 3, s)
        else:
            close(host[s], O.neighbourhood(f, 3, s), exact=s not in (gridpp.Mean, gridpp.Sum))
    same(hq[0], O.neighbourhood_quantile_fast(f, [0.5], 4, thr))
    same(hq[1], O.neighbourhood_quantile_fast(f, qf, 2, thr))
    flat = torch.from_numpy(f.ravel())
    for off in (1, 2, 3):
        base = torch.zeros(flat.numel() + 8, dtype=torch.float32, device="cuda")
        d = base[off:off + flat.numel()]
        d.copy_(flat)
        d = d.view(f.shape)
        assert d.data_ptr() % 16 != 0 and d.is_contiguous()
        for s in stats:
            identical(gridpp.neighbourhood(d, 3, s).cpu().numpy(), host[s])
        identical(gridpp.neighbourhood_quantile_fast(d, 0.5, 4, thr).cpu().numpy(), hq[0])
        identical(gridpp.neighbourhood_quantile_fast(d, torch.from_numpy(qf).cuda(), 2, thr).cpu().numpy(), hq[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. quantile_fast on both sides of every limit of the fused path (E <= 254, T <= 16, halfwidth <= 16; ranks for E % 4 == 0)
# ---------------------------------------------------------------------------------------------------------------------------------
QF_CASES = [   # (E, T, hw, invalid members, X); Y = 37, so no field is a whole number of 64-cell tiles
    (1, 15, 0, True, 45), (1, 17, 16, False, 44),
    (3, 16, 15, False, 46), (3, 17, 17, True, 45),
    (4, 16, 16, True, 44), (4, 15, 17, False, 47),
    (64, 16, 15, False, 45), (64, 17, 16, True, 44),
    (161, 16, 0, True, 45), (161, 15, 17, False, 46),
    (200, 16, 15, True, 47), (200, 17, 16, False, 44),
    (252, 15, 16, False, 45), (252, 16, 0, True, 44),
    (253, 16, 15, False, 44),
    (254, 16, 16, True, 45), (254, 17, 15, False, 46),
    (255, 16, 16, False, 45),
    (256, 16, 15, True, 44), (256, 15, 17, False, 45),
]


@pytest.mark.parametrize("E,T,hw,invalid,X", QF_CASES)
def test_quantile_fast_at_the_fused_limits(api, E, T, hw, invalid, X):
    """Ranked (k_qf_count) and compare-per-threshold (k_member_pass<2>) byte counts, from LDS (E <= 160) and from memory; the
    unfused form (k_member_pass<1> + box pass with the E-fold epilogue) just beyond each limit; rows with and without invalid
    members (the box pass's rowflag path on / off), X % 4 != 0.  Members sit on the thresholds in every other case.  A scalar
    quantile and a quantile field holding 0, 1 and NaN."""
    gridpp, O = api
    Y = 37
    rng = np.random.default_rng(E * 1000 + T * 10 + hw)
    f = rng.uniform(-1, T + 1, (Y, X, E))
    if E % 2 == 0:
        f = np.round(f)
    f = f.astype(np.float32)
    if invalid:
        f[rng.random(f.shape) < 0.02] = np.nan
        f[rng.random(f.shape) < 0.01] = np.inf
        f[3:5, 7:9, :] = np.nan
    thr = np.arange(T, dtype=np.float32)
    q = (0.5, 0.0, 1.0, 0.9, 0.1)[(E + T + hw) % 5]
    same(gridpp.neighbourhood_quantile_fast(f, q, hw, thr), O.neighbourhood_quantile_fast(f, [q], hw, thr))
    qf = rng.random((Y, X)).astype(np.float32)
    qf[0, :5] = 0.0
    qf[1, :5] = 1.0
    qf[2, :5] = np.nan
    same(gridpp.neighbourhood_quantile_fast(f, qf, hw, thr), O.neighbourhood_quantile_fast(f, qf, hw, thr))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the lazy E-fold sums of the box pass (qf_box.hip) where the margin is tight
# ---------------------------------------------------------------------------------------------------------------------------------
def fold(o, E):
    """F(o): the reference's E-fold float32 sum of a window mean, / E, clamped to [0, 1] (neighbourhood.cpp:494-506)"""
    o = np.asarray(o, np.float32)
    s = np.zeros_like(o)
    for _ in range(E):
        s = (s + o).astype(np.float32)
    return np.clip((s / np.float32(E)).astype(np.float32), np.float32(0), np.float32(1))


def window_means(f, thr, hw):
    """o_t of every cell and threshold as the box pass forms it: temp = (float)count / valid per cell, the exact sum of the temps of the
    window (they are multiples of 2^-32 below 2^12 here: float64 holds every partial sum), divided in float64 and rounded to float32"""
    Y, X, E = f.shape
    valid = (~np.isnan(f) & ~np.isinf(f)).sum(-1)
    assert (valid == E).all()
    temp = np.stack([((f <= t).sum(-1).astype(np.float32) / np.float32(E)).astype(np.float32) for t in thr]).astype(np.float64)
    S = np.zeros((len(thr), Y + 1, X + 1))
    S[:, 1:, 1:] = temp.cumsum(1).cumsum(2)
    y0, y1 = np.clip(np.arange(Y) - hw, 0, Y), np.clip(np.arange(Y) + hw + 1, 0, Y)
    x0, x1 = np.clip(np.arange(X) - hw, 0, X), np.clip(np.arange(X) + hw + 1, 0, X)
    win = S[:, y1][:, :, x1] - S[:, y0][:, :, x1] - S[:, y1][:, :, x0] + S[:, y0][:, :, x0]
    n = (y1 - y0)[:, None] * (x1 - x0)[None, :]
    return (win / n).astype(np.float32)


def strictly_between(o, F):
    """a float32 strictly between o and F (their midpoint, moved inside), NaN where no float lies between them"""
    lo, hi = np.minimum(o, F), np.maximum(o, F)
    m = ((lo.astype(np.float64) + hi) / 2).astype(np.float32)
    m = np.where(m <= lo, np.nextafter(lo, np.float32(2)), m)
    return np.where((m > lo) & (m < hi), m, np.float32(np.nan)).astype(np.float32)


@pytest.mark.parametrize("E", [200, 252, 254])
def test_lazy_margin_where_it_is_tight(api, E):
    """qb_interp_lazy forms F(o) only for thresholds whose window mean o is within 1.2e-5 o of the quantile x (its proof bounds
    |F(o) - o| by 7.7e-6 o; at these E the helper finds up to 3.8e-6 o).  window_means and fold reproduce o and F(o) exactly on
    integer-valued members, so the quantiles below are placed relative to them.  Two kinds of case, each in hundreds of cells:
    (a) a discontinuity.  Members are even integers, the thresholds all integers: thresholds 2k and 2k + 1 have the same counts,
    F_2k == F_2k+1 is a plateau, and interpolate() jumps by a whole threshold step where x crosses it.  With x strictly between o_2k
    and F(o_2k) -- a few 1e-6 from o -- the reference lands on one side of the jump; a path that decides the side on o lands on
    the other, one step away: the oracle comparison alone catches it.  (The variant with q = 1 and F(o_0) = 1 > o_0 does not exist:
    F(o) < 1 for every float o < 1 at every E <= 254, asserted below over the whole range where |F(o) - o| <= 7.7e-6 o allows F = 1.)
    (b) a bracket shift without a plateau.  x strictly between o_t and F(o_t) in a field of all integers: interpolation is continuous
    across the shift, so the 1e-5 of the oracle cannot see a wrong bracket.  The fused form is compared with the unfused one
    (GPP_QF_NO_FUSED: F at every threshold, k_box_march's epilogue + k_qf_interp) and the unranked one (GPP_QF_NO_RANKS): the same
    window means from the same exact sums and the same E-fold float sums -- measured bit-identical on every cell, asserted so."""
    gridpp, O = api
    # F(o) < 1 for o < 1 at every E <= 254: o = 1 - m 2^-24, m = 1 .. 130 covers 1 - 7.7e-6 <= o < 1 (the running sum after k terms is
    # the E-fold sum of E = k)
    o_hi = (1.0 - np.arange(1, 131) * U32).astype(np.float32)
    s = np.zeros_like(o_hi)
    for k in range(1, 255):
        s = (s + o_hi).astype(np.float32)
        assert ((s / np.float32(k)).astype(np.float32) < 1).all(), k
    Y, X, T, hw = 48, 50, 16, 11
    thr = np.arange(T, dtype=np.float32)
    rng = np.random.default_rng(E)
    cells = np.arange(Y * X).reshape(Y, X)
    # (a) even members: plateaus F_2k == F_2k+1
    f = (2 * np.floor(rng.uniform(0, 8, (Y, X, E)) ** rng.uniform(0.6, 1.4, (Y, X, 1)))).astype(np.float32)
    o = window_means(f, thr, hw)
    t = 2 * (cells % 7)                                          # the threshold whose plateau the quantile of the cell sits against
    ot = np.take_along_axis(o, t[None], 0)[0]
    x = strictly_between(ot, fold(ot, E))
    hit = ~np.isnan(x) & (np.abs(x.astype(np.float64) - ot) > 1e-6 * ot)
    assert hit.sum() > 200, hit.sum()
    q = np.where(hit, x, rng.random((Y, X)).astype(np.float32))
    out = gridpp.neighbourhood_quantile_fast(f, q, hw, thr)
    ref = O.neighbourhood_quantile_fast(f, q, hw, thr)
    same(out, ref)
    # (b) all integers 0 .. 15: no plateau
    g = np.floor(rng.uniform(0, T, (Y, X, E)) ** rng.uniform(0.7, 1.0, (Y, X, 1))).astype(np.float32)
    o = window_means(g, thr, hw)
    t = 1 + cells % (T - 2)
    ot = np.take_along_axis(o, t[None], 0)[0]
    x = strictly_between(ot, fold(ot, E))
    hit = ~np.isnan(x) & (np.abs(x.astype(np.float64) - ot) > 1e-6 * ot)
    assert hit.sum() > 200, hit.sum()
    q = np.where(hit, x, rng.random((Y, X)).astype(np.float32))
    fused = gridpp.neighbourhood_quantile_fast(g, q, hw, thr)
    same(fused, O.neighbourhood_quantile_fast(g, q, hw, thr))
    with override(gridpp, "GPP_QF_NO_FUSED"):
        identical(fused, gridpp.neighbourhood_quantile_fast(g, q, hw, thr))
    with override(gridpp, "GPP_QF_NO_RANKS"):
        identical(fused, gridpp.neighbourhood_quantile_fast(g, q, hw, thr))
    # one-ulp quantiles next to the means: no discrimination (inside any margin), extra coverage of the equality branches
    q1 = np.nextafter(ot, np.float32(1)).astype(np.float32)
    fused = gridpp.neighbourhood_quantile_fast(g, q1, hw, thr)
    same(fused, O.neighbourhood_quantile_fast(g, q1, hw, thr))
    with override(gridpp, "GPP_QF_NO_FUSED"):
        identical(fused, gridpp.neighbourhood_quantile_fast(g, q1, hw, thr))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. call sequences: the speculative count pass and the padding cache of the count planes
# ---------------------------------------------------------------------------------------------------------------------------------
def test_call_sequence_speculation_and_padding_cache(api):
    """The count pass is launched for the number of distinct thresholds the last call with as many thresholds had (spec_nt / spec_U),
    stopped on the device when this call's table differs, and run again; a device-resident quantile is validated after the kernels.
    The padding of the count planes is laid out once per (buffer, allocation, Y, X, T, E).  Each step equals the oracle and the same
    call with GPP_QF_NO_SPEC (which waits for the table, and leaves the speculation state the speculative call leaves)."""
    import torch
    gridpp, O = api
    T = 8
    A = np.linspace(0, 10, T).astype(np.float32)      # U = T
    B = A.copy()
    B[5] = B[2]                                       # a duplicate: U = T - 1
    Cl = A.copy()
    Cl[4] = np.nextafter(Cl[3], np.float32(np.inf))   # two thresholds in one bucket: the table's flag
    f8 = field(50, 31, 60, 8)
    f12 = field(51, 31, 60, 12)
    g12 = field(52, 23, 70, 12)   # (23 + 33) * 128 == (31 + 33) * 112 bytes per count plane: the same buffer, another layout
    qf = np.random.default_rng(6).random((31, 60)).astype(np.float32)

    def step(f, thr, q=0.5, hw=4):
        out = gridpp.neighbourhood_quantile_fast(f, q, hw, thr)
        with override(gridpp, "GPP_QF_NO_SPEC"):
            ref = gridpp.neighbourhood_quantile_fast(f, q, hw, thr)
        identical(out, ref)
        same(out, O.neighbourhood_quantile_fast(f, [q] if np.ndim(q) == 0 else q, hw, thr))

    with override(gridpp, "GPP_QF_NO_SPEC"):
        gridpp.neighbourhood_quantile_fast(f8, 0.5, 4, A)          # the speculation state: (T, T)
    step(f8, A)                 # speculation hit
    step(f8, B, qf)             # miss: launched for U = T, the table has T - 1
    step(f8, Cl)                # miss: the table is flagged (compare-per-threshold pass); the state is forgotten
    step(f8, A, qf, 16)         # no speculation, the state is (T, T) again
    step(f8, A, 0.9, 0)         # hit
    step(f12, A)                # only E changed: the padding is laid out again
    step(g12, A, 0.3, 7)        # only the shape changed, the same plane bytes
    # a device-resident quantile field outside [0, 1]: rejected before the kernels (no speculation) and after them (speculation)
    dg, dthr = torch.from_numpy(g12).cuda(), torch.from_numpy(A).cuda()
    good = torch.from_numpy(np.random.default_rng(7).random((23, 70)).astype(np.float32)).cuda()
    bad = good.clone()
    bad[3, 4] = 1.5
    want = O.neighbourhood_quantile_fast(g12, good.cpu().numpy(), 4, A)
    gridpp.neighbourhood_quantile_fast(g12, 0.5, 4, Cl)              # flagged: forgets the state
    with pytest.raises(ValueError):
        gridpp.neighbourhood_quantile_fast(dg, bad, 4, dthr)
    first = gridpp.neighbourhood_quantile_fast(dg, good, 4, dthr).cpu().numpy()   # no speculation: the state is (T, T) again
    with pytest.raises(ValueError):
        gridpp.neighbourhood_quantile_fast(dg, bad, 4, dthr)            # speculation: validated behind the kernels
    after = gridpp.neighbourhood_quantile_fast(dg, good, 4, dthr).cpu().numpy()
    with override(gridpp, "GPP_QF_NO_SPEC"):
        plain = gridpp.neighbourhood_quantile_fast(dg, good, 4, dthr).cpu().numpy()
    for r in (first, after):
        identical(r, plain)
        same(r, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. calc_statistic / calc_quantile on long rows (member pass up to 160, k_rows_statistic / k_rows_quantile beyond and for quantiles)
# ---------------------------------------------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 3, 4, 5, 159, 160, 161, 300, 1000]
QUANTILES = [0.0, 1e-7, 0.5, float(np.float32(1 - 2.0 ** -24)), 1.0, float("nan")]


def rows(L, R=70):
    """R rows of L members (70: a partial second tile): NaN / +-inf members, an all-invalid row, duplicates, +-0.0, a constant row,
    a large offset with a small spread"""
    rng = np.random.default_rng(L)
    a = rng.uniform(-10, 10, (R, L)).astype(np.float32)
    r = rng.random(a.shape)
    a[r < 0.05] = np.nan
    a[(r >= 0.05) & (r < 0.07)] = np.inf
    a[(r >= 0.07) & (r < 0.09)] = -np.inf
    a[1] = np.nan
    a[2] = np.where(np.arange(L) % 2, np.inf, -np.inf)
    a[3] = rng.integers(-3, 4, L)
    a[4] = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0], np.float32), L)
    a[5] = 7.25
    a[6] = 1e4 + rng.uniform(0, 1, L)
    a[7:20, ::3] = a[7:20, :1]
    a[20, ::2] = -0.0
    return a


def bit_equal(a, b, zero_sign=False):
    """a == b bit for bit (NaN: NaN-ness).  zero_sign: a zero may have either sign (see test_long_rows)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    assert (na == nb).all()
    diff = (a.view(np.uint32) != b.view(np.uint32)) & ~na
    if zero_sign:
        diff &= ~((a == 0) & (b == 0))
    assert not diff.any(), (np.nonzero(diff)[0][:5], a[diff][:5], b[diff][:5])


def numpy_check(row, stat_or_q, got, gridpp):
    """A second opinion in float64 (numpy on the finite members), within a bound from the row length n (unit roundoff u = 2^-24):
    sequential float sums within (n - 1) u sum|x| (+ u of the quotient for a mean); the shifted variance of the reference within
    (3 n + 7) u E[(x - K)^2] (Std: the same bound on its square, + 3 u Std^2); a quantile within (6 n + 2) u times the gap of the order
    statistics around its index (the float index q (n - 1) and the float weights) + 2 u |value|."""
    x = row[np.isfinite(row)].astype(np.float64)
    n = x.size
    got = float(got)
    if isinstance(stat_or_q, float):
        q = stat_or_q
        if n == 0 or np.isnan(q):
            assert np.isnan(got)
            return
        s = np.sort(x)
        want = float(np.quantile(x, q, method="linear"))
        k = int(np.floor(q * (n - 1)))
        gap = s[min(k + 2, n - 1)] - s[max(k - 1, 0)]
        assert abs(got - want) <= gap * (6 * n + 2) * U32 + 2 * U32 * abs(want) + 1e-30, (q, n, got, want)
        return
    stat = stat_or_q
    if stat == gridpp.Count:
        assert got == n
        return
    if n == 0:
        assert np.isnan(got)
        return
    g = 1.01 * n * U32
    if stat == gridpp.Sum:
        assert abs(got - x.sum()) <= g * np.abs(x).sum()
    elif stat == gridpp.Mean:
        assert abs(got - x.mean()) <= g * np.abs(x).mean() + 1.01 * U32 * abs(x.mean())
    elif stat == gridpp.Min:
        assert got == x.min()
    elif stat == gridpp.Max:
        assert got == x.max()
    elif stat == gridpp.Median:
        numpy_check(row, 0.5, got, gridpp)
    else:
        m2 = np.mean((x - x[0]) ** 2)
        bound = 1.01 * (3 * n + 7) * U32 * m2
        var = np.var(x)
        if stat == gridpp.Variance:
            assert abs(got - var) <= bound, (got, var, bound)
        else:
            assert abs(got * got - var) <= bound + 3 * U32 * got * got, (got, var, bound)


@pytest.mark.parametrize("L", LENGTHS)
def test_long_rows(api, L):
    """gridpp.calc_statistic / calc_quantile per row against O.calc_statistic / O.calc_quantile row by row: bit for bit -- both run
    the reference's sequential float loops (row_stats.h) -- except for the sign of a zero Median / quantile: the reference sorts with
    std::sort, under which -0.0 and +0.0 are equivalent and their order is unspecified, while row_kth's bisection ranks -0.0 below +0.0.
    Also against numpy in float64 within a bound from the row length (numpy_check)."""
    gridpp, O = api
    a = rows(L)
    stats = (gridpp.Mean, gridpp.Sum, gridpp.Count, gridpp.Min, gridpp.Max, gridpp.Std, gridpp.Variance, gridpp.Median)
    for stat in stats:
        got = gridpp.calc_statistic(a, stat)
        bit_equal(got, [O.calc_statistic(r, stat) for r in a], zero_sign=stat == gridpp.Median)
        for r, v in zip(a, got):
            numpy_check(r, stat, v, gridpp)
    for q in QUANTILES:
        got = gridpp.calc_quantile(a, q)
        bit_equal(got, [O.calc_quantile(r, q) for r in a], zero_sign=q not in (0.0, 1.0))
        for r, v in zip(a, got):
            numpy_check(r, q, v, gridpp)
    # the (vec3, vec2 quantile) overload: a quantile per row
    a3 = a.reshape(7, 10, L)
    q2 = np.array(QUANTILES * 12, np.float32)[:70].reshape(7, 10)
    got = gridpp.calc_quantile(a3, q2)
    bit_equal(got.ravel(), [O.calc_quantile(r, q) for r, q in zip(a, q2.ravel())], zero_sign=True)
    for r, q, v in zip(a, q2.ravel(), got.ravel()):
        numpy_check(r, float(q), v, gridpp)
