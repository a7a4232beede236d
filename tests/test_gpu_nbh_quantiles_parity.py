"""gridpp_amd.neighbourhood_quantiles_fast and neighbourhood_cdf on the GPU.

Every level plane has the bits of the single-level neighbourhood_quantile_fast, on the fused path (k_qf_box_multi: plain and GENERAL
kernels, every halfwidth class, one and several strips and row segments, one and several launches of levels) and on every other path;
every plane agrees with the oracle; neighbourhood_cdf agrees with the numpy restatement of the reference's yarray (tests/nbh_cdf_ref.py,
pinned to the oracle by tests/test_nbh_quantiles_api.py); the chain cdf -> interpolate gives the quantile bit for bit; and the calls
leave each other's state (count planes, padding cache, speculation) intact."""
import numpy as np
import pytest

from tests import nbh_cdf_ref
from tests.test_gpu_neighbourhood_edges import identical, members, override, same
from tests.test_gpu_neighbourhood_parity import close, field

pytestmark = pytest.mark.gpu
F = np.float32
LEVELS = np.array([0, 0.1, 0.5, 0.5, 0.500001, 0.9, 1, np.nan], F)


@pytest.fixture(scope="module")
def api():
    import gridpp_amd as gridpp
    from oracle import oracle as O
    return gridpp, O


def cube(seed, shape, missing):
    """uniform [0, 10) members (tests.test_gpu_neighbourhood_parity.field); missing: NaN members and cells with none valid, down to the smallest shape"""
    Y, X, E = shape
    f = field(seed, Y, X, E, nan_blocks=missing)
    if missing:
        f[0, 0, 0] = np.nan
        f[Y // 2, X // 2, :] = np.inf
    return f


def planes_equal_single_calls(gridpp, f, levels, hw, thr):
    out = gridpp.neighbourhood_quantiles_fast(f, levels, hw, thr)
    assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == f.shape[:2] + (len(levels),)
    for j, q in enumerate(levels):
        identical(np.ascontiguousarray(out[:, :, j]), gridpp.neighbourhood_quantile_fast(f, float(q), hw, thr))
    return out


# ---- 1. every level plane has the bits of the single-level call: the fused path ---------------------------------------------------------------
@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 4), (5, 3, 4), (33, 65, 20), (70, 300, 8), (700, 70, 4)])
def test_level_planes_equal_the_single_level_call(api, shape, missing):
    """(70, 300, 8): two 256-column strips, the second partial; (700, 70, 4): many row segments (GPP_QB_FILL).  missing: the GENERAL kernel (rows
    with cells of fewer than E valid members), else the plain one.  T = 11 over uniform [0, 10) members is the ambiguous case of qb_interp_lazy's
    comment: integer thresholds 0 .. 10, q = 0.5 on the expected rank of threshold 5 -- window means sit on the level."""
    gridpp, O = api
    f = cube(100 + shape[0], shape, missing)
    for hw in (0, 4, 15, 16):
        for T in (1, 2, 11, 16):
            thr = np.linspace(0, 10, T).astype(F)
            out = planes_equal_single_calls(gridpp, f, LEVELS, hw, thr)
            assert np.isnan(out[:, :, 7]).all()
            identical(np.ascontiguousarray(out[:, :, 2]), np.ascontiguousarray(out[:, :, 3]))


@pytest.mark.parametrize("Q", [1, 2, 31, 32, 33, 70])
def test_levels_on_both_sides_of_the_per_launch_limit(api, Q):
    """the box pass takes 32 levels per launch (QB_MAXQ): 33 and 70 levels are two and three launches writing their columns of one result"""
    gridpp, O = api
    rng = np.random.default_rng(Q)
    levels = rng.random(Q).astype(F)
    levels[0] = 0.5
    for missing in (False, True):
        f = cube(7, (40, 270, 8), missing)
        planes_equal_single_calls(gridpp, f, levels, 3, np.linspace(0, 10, 11).astype(F))


def test_one_level_is_the_single_level_result(api):
    gridpp, O = api
    f = cube(8, (33, 65, 20), True)
    thr = np.linspace(0, 10, 11).astype(F)
    out = gridpp.neighbourhood_quantiles_fast(f, [0.5], 15, thr)
    assert out.shape == (33, 65, 1)
    identical(out[:, :, 0], gridpp.neighbourhood_quantile_fast(f, 0.5, 15, thr))


# ---- 2. the other paths --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["E7_compare_pass", "E255_unfused", "T17_unfused", "hw17_unfused", "2d"])
def test_level_planes_on_the_other_paths(api, case):
    gridpp, O = api
    E, T, hw = {"E7_compare_pass": (7, 11, 4), "E255_unfused": (255, 5, 3), "T17_unfused": (8, 17, 4), "hw17_unfused": (8, 11, 17), "2d": (None, 11, 4)}[case]
    thr = np.linspace(0, 10, T).astype(F)
    for missing in (False, True):
        if E is None:
            f = field(31, 70, 300, nan_blocks=missing)
        elif E == 255:
            f = cube(32, (20, 40, 255), missing)
        else:
            f = cube(33, (70, 300, E), missing)
        out = planes_equal_single_calls(gridpp, f, LEVELS, hw, thr)
        for j in (1, 2, 6):
            close(np.ascontiguousarray(out[:, :, j]), O.neighbourhood_quantile_fast(f, [LEVELS[j]], hw, thr))
    g = members(34, 40, 70, 8 if E in (None, 255) else E)       # offsets and scales that vary from cell to cell, +-inf members
    thr = np.linspace(-20, 40, T).astype(F)
    planes_equal_single_calls(gridpp, g[:, :, 0].copy() if E is None else g, LEVELS, hw, thr)


@pytest.mark.parametrize("name", ["GPP_QF_NO_FUSED", "GPP_QF_NO_RANKS", "GPP_QF_NO_SPEC"])
def test_path_overrides_act_on_the_new_entries(api, name):
    """under each override the level planes equal the single-level call under the same override, and the result of the default path"""
    gridpp, O = api
    thr = np.linspace(0, 10, 11).astype(F)
    for missing in (False, True):
        f = cube(41, (70, 300, 8), missing)
        default = gridpp.neighbourhood_quantiles_fast(f, LEVELS, 4, thr)
        default_cdf = gridpp.neighbourhood_cdf(f, thr, 4)
        with override(gridpp, name):
            out = planes_equal_single_calls(gridpp, f, LEVELS, 4, thr)
            out2 = planes_equal_single_calls(gridpp, f, LEVELS, 4, thr)      # (a second call: GPP_QF_NO_SPEC keeps it from speculating)
            cdf = gridpp.neighbourhood_cdf(f, thr, 4)
        identical(out, out2)
        if name == "GPP_QF_NO_FUSED":     # the two-pass box sums add the same doubles in another order (test_fused_box_pass_against_the_two_pass_form's measure)
            assert (np.isnan(cdf) == np.isnan(default_cdf)).all() and (np.isnan(out) == np.isnan(default)).all()
            m = ~np.isnan(default_cdf)
            assert (np.abs(cdf[m].astype(np.float64) - default_cdf[m]) <= 1e-6 * np.maximum(np.abs(default_cdf[m]), 1e-3)).all()
        else:
            identical(out, default)
            identical(cdf, default_cdf)


@pytest.mark.parametrize("kind", ["permuted", "duplicate", "clustered", "nonfinite", "integer_ties"])
def test_threshold_lists(api, kind):
    """the lists of test_quantile_fast_threshold_lists: level planes bit for bit with the single-level call and against the oracle (`same`:
    infinities exactly), cdf planes against the restatement, in the order the thresholds are given"""
    gridpp, O = api
    rng = np.random.default_rng(21)
    f = rng.uniform(0, 10, (90, 300, 8)).astype(F)
    f[rng.random(f.shape) < 0.01] = np.nan
    f[70:73, 100:110, :] = np.nan
    thr = np.linspace(0, 10, 9).astype(F)
    if kind == "permuted":
        thr = rng.permutation(thr)
    elif kind == "duplicate":
        thr[3] = thr[5]
    elif kind == "clustered":
        thr[4] = np.nextafter(thr[3], F(np.inf))
    elif kind == "nonfinite":
        thr[2], thr[7] = np.inf, np.nan
    else:
        f = np.round(f).astype(F)
    levels = np.array([0.5, 0.9, 0.0, 1.0], F)
    for hw in (15, 3):
        out = planes_equal_single_calls(gridpp, f, levels, hw, thr)
        for j, q in enumerate(levels):
            same(np.ascontiguousarray(out[:, :, j]), O.neighbourhood_quantile_fast(f, [q], hw, thr))
        close(gridpp.neighbourhood_cdf(f, thr, hw), nbh_cdf_ref.cdf(O, f, thr, hw))
    g = f[:, :, :7].copy()   # rows that are no whole float4s: the compare-per-threshold pass feeds the same box pass
    out = planes_equal_single_calls(gridpp, g, levels, 7, thr)
    same(np.ascontiguousarray(out[:, :, 0]), O.neighbourhood_quantile_fast(g, [0.5], 7, thr))


# ---- 3. against the oracle directly ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,hw,T", [((33, 65, 20), 15, 11), ((70, 300, 8), 4, 16), ((5, 3, 4), 16, 2), ((40, 50, 6), 2, 11)])
def test_level_planes_against_the_oracle(api, shape, hw, T):
    gridpp, O = api
    thr = np.linspace(0, 10, T).astype(F)
    for missing in (False, True):
        f = cube(51, shape, missing)
        out = gridpp.neighbourhood_quantiles_fast(f, LEVELS, hw, thr)
        for j, q in enumerate(LEVELS):
            close(np.ascontiguousarray(out[:, :, j]), O.neighbourhood_quantile_fast(f, [q], hw, thr))       # every cell, NaN where the oracle is NaN
    thr = np.array([-np.inf, 2.0, 5.0, np.inf], F)
    f = cube(52, shape, True)
    out = gridpp.neighbourhood_quantiles_fast(f, LEVELS, hw, thr)
    for j, q in enumerate(LEVELS):
        same(np.ascontiguousarray(out[:, :, j]), O.neighbourhood_quantile_fast(f, [q], hw, thr))


# ---- 4. neighbourhood_cdf ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,hw", [((1, 1, 4), 0), ((5, 3, 4), 4), ((33, 65, 20), 15), ((70, 300, 8), 16), ((700, 70, 4), 4), ((70, 300, 7), 4), ((20, 40, 255), 3),
                                      ((70, 300, 8), 17), ((70, 300), 4), ((70, 300), 20)])
def test_cdf_against_the_restatement(api, shape, hw):
    """fused (plain and GENERAL kernels), the compare pass (E = 7), unfused (E = 255, halfwidth 17, T = 17) and 2-D input.  The reference's Mean is
    a double summed-area table, the box pass adds exact doubles: the two differ by the float32 rounding of one quotient."""
    gridpp, O = api
    rng = np.random.default_rng(61)
    for missing in (False, True):
        f = cube(60, shape, missing) if len(shape) == 3 else field(60, shape[0], shape[1], nan_blocks=missing)
        for T in (1, 11, 16, 17):
            thr = np.linspace(0, 10, T).astype(F)
            ref = nbh_cdf_ref.cdf(O, f, thr, hw)
            out = gridpp.neighbourhood_cdf(f, thr, hw)
            assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == f.shape[:2] + (T,)
            close(out, ref)                                            # (NaN exactly where the restatement is NaN)
            ok = ~np.isnan(out)
            assert (out[ok] >= 0).all() and (out[ok] <= 1).all()
            perm = rng.permutation(T)                                  # the planes follow the thresholds as given
            identical(gridpp.neighbourhood_cdf(f, thr[perm], hw), np.ascontiguousarray(out[:, :, perm]))
    assert gridpp.neighbourhood_cdf(f, [], hw).shape == f.shape[:2] + (0,)


def test_cdf_windows_without_a_valid_cell_and_odd_thresholds(api):
    gridpp, O = api
    f = cube(62, (40, 70, 8), True)
    f[10:30, 20:50, :] = np.nan
    thr = np.array([np.nan, 5.0, np.inf, 5.0, -np.inf, 2.0], F)         # non-finite and duplicated thresholds, unsorted
    for hw in (0, 2, 16):
        ref = nbh_cdf_ref.cdf(O, f, thr, hw)
        out = gridpp.neighbourhood_cdf(f, thr, hw)
        close(out, ref)
        if hw <= 2:
            assert np.isnan(out[20, 35]).all() and not np.isnan(out[0, 0]).any()
        ok = ~np.isnan(out[:, :, 0])
        assert (out[:, :, 0][ok] == 0).all() and (out[:, :, 2][ok] == 1).all() and (out[:, :, 4][ok] == 0).all()     # nothing is <= NaN or -inf, every valid member is <= inf
        identical(np.ascontiguousarray(out[:, :, 1]), np.ascontiguousarray(out[:, :, 3]))


@pytest.mark.parametrize("shape,hw", [((33, 65, 20), 15), ((70, 300, 8), 4), ((700, 70, 4), 16)])
def test_cdf_fused_against_unfused(api, shape, hw):
    """The project's fused-versus-two-pass test (test_fused_box_pass_against_the_two_pass_form) holds the two forms of the box Mean to 1e-6 relative
    over a floor of 1e-3, not to the bit (the same doubles added in another order); the cdf is such a Mean, folded and clamped: the same bound."""
    gridpp, O = api
    thr = np.linspace(0, 10, 11).astype(F)
    for missing in (False, True):
        f = cube(63, shape, missing)
        fused = gridpp.neighbourhood_cdf(f, thr, hw)
        with override(gridpp, "GPP_QF_NO_FUSED"):
            two = gridpp.neighbourhood_cdf(f, thr, hw)
        assert (np.isnan(fused) == np.isnan(two)).all()
        m = ~np.isnan(two)
        assert (np.abs(fused[m].astype(np.float64) - two[m]) <= 1e-6 * np.maximum(np.abs(two[m]), 1e-3)).all()


# ---- 5. the tie between the two ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(33, 65, 20), (70, 300, 8)])
def test_interpolating_in_the_cdf_gives_the_quantile_bit_for_bit(api, shape):
    """interpolate(q, cdf[y, x, :], thresholds) with the two special cases of neighbourhood.cpp:514-517, in float32 (numpy: no contraction), has the bits
    of neighbourhood_quantile_fast wherever the column holds no NaN, and the quantile is NaN where it does"""
    gridpp, O = api
    for missing in (False, True):
        f = cube(71, shape, missing)
        for hw, T in ((15, 11), (4, 16), (0, 2)):
            thr = np.linspace(0, 10, T).astype(F)
            ya = gridpp.neighbourhood_cdf(f, thr, hw)
            for q in (0.0, 0.3, 0.5, 1.0):
                identical(nbh_cdf_ref.quantile_from_cdf(ya, thr, q), gridpp.neighbourhood_quantile_fast(f, q, hw, thr))
    g = members(72, shape[0], shape[1], shape[2])
    thr = np.linspace(-20, 40, 11).astype(F)
    ya = gridpp.neighbourhood_cdf(g, thr, 4)
    for q in (0.0, 0.3, 0.5, 1.0):
        identical(nbh_cdf_ref.quantile_from_cdf(ya, thr, q), gridpp.neighbourhood_quantile_fast(g, q, 4, thr))


# ---- 6. state ------------------------------------------------------------------------------------------------------------------------------------
def test_calls_leave_each_others_state_intact(api):
    """single-level, many-level and cdf calls share the count planes, their padding cache and the speculation: every call of an interleaved sequence
    returns what the same call returns as the first one after the workspaces were released"""
    gridpp, O = api
    f = cube(81, (70, 300, 8), True)
    g = cube(82, (33, 65, 8), False)
    thr = np.linspace(0, 10, 11).astype(F)
    other = np.linspace(1, 9, 11).astype(F)      # as many thresholds, other values: the speculation fails and the plain round follows
    levels = [0.1, 0.5, 0.9]
    calls = [lambda: gridpp.neighbourhood_quantile_fast(f, 0.5, 15, thr),
             lambda: gridpp.neighbourhood_quantiles_fast(f, levels, 15, thr),
             lambda: gridpp.neighbourhood_cdf(f, thr, 15),
             lambda: gridpp.neighbourhood_quantiles_fast(f, levels, 15, other),
             lambda: gridpp.neighbourhood_quantiles_fast(g, levels, 4, thr),      # another shape: the padding cache is invalidated
             lambda: gridpp.neighbourhood_cdf(g, other, 4),
             lambda: gridpp.neighbourhood_quantile_fast(f, 0.5, 15, thr),
             lambda: gridpp.neighbourhood_quantiles_fast(f, levels, 15, thr),
             lambda: gridpp.neighbourhood_cdf(f, thr, 15)]
    fresh = []
    for call in calls:
        gridpp.release_workspaces()
        fresh.append(call())
    gridpp.release_workspaces()
    for _ in range(2):
        for call, want in zip(calls, fresh):
            identical(call(), want)
    for call, want in zip(reversed(calls), reversed(fresh)):
        identical(call(), want)


def test_device_tensors_and_float64(api):
    import torch
    gridpp, O = api
    thr = np.linspace(0, 10, 11).astype(F)
    levels = [0.1, 0.5, 0.9, np.nan]
    for f, hw in ((cube(91, (70, 300, 8), True), 15), (cube(92, (70, 300, 8), True), 17), (field(93, 70, 300), 4)):
        d = torch.from_numpy(f).cuda()
        out = gridpp.neighbourhood_quantiles_fast(d, levels, hw, thr)
        assert out.is_cuda and out.device == d.device and out.dtype == torch.float32 and tuple(out.shape) == f.shape[:2] + (4,)
        identical(out.cpu().numpy(), gridpp.neighbourhood_quantiles_fast(f, levels, hw, thr))
        cdf = gridpp.neighbourhood_cdf(d, torch.from_numpy(thr).cuda(), hw)
        assert cdf.is_cuda and cdf.device == d.device and tuple(cdf.shape) == f.shape[:2] + (11,)
        identical(cdf.cpu().numpy(), gridpp.neighbourhood_cdf(f, thr, hw))
        assert tuple(gridpp.neighbourhood_quantiles_fast(d, [], hw, thr).shape) == f.shape[:2] + (0,)
        # a float64 cube gives the bits of its float32 cast
        identical(gridpp.neighbourhood_quantiles_fast(f.astype(np.float64), levels, hw, thr), gridpp.neighbourhood_quantiles_fast(f, levels, hw, thr))
        identical(gridpp.neighbourhood_cdf(f.astype(np.float64), thr, hw), gridpp.neighbourhood_cdf(f, thr, hw))
    # a float64 cube large enough to travel as float64 (GPP_HOST_F64: cast on the device), with values that are no float32s
    rng = np.random.default_rng(94)
    big = rng.uniform(0, 10, (128, 1100, 8))
    big[rng.random(big.shape) < 0.01] = np.nan
    assert big.size >= 1 << 20
    identical(gridpp.neighbourhood_quantiles_fast(big, levels, 4, thr), gridpp.neighbourhood_quantiles_fast(big.astype(F), levels, 4, thr))
    identical(gridpp.neighbourhood_cdf(big, thr, 4), gridpp.neighbourhood_cdf(big.astype(F), thr, 4))


def test_no_thresholds_and_no_levels(api):
    gridpp, O = api
    f = cube(95, (33, 65, 20), True)
    out = gridpp.neighbourhood_quantiles_fast(f, [0.1, 0.5], 4, [])
    assert out.shape == (33, 65, 2) and out.dtype == F and np.isnan(out).all()
    assert gridpp.neighbourhood_quantiles_fast(f, [], 4, [1.0, 2.0]).shape == (33, 65, 0)
    assert gridpp.neighbourhood_cdf(f, [], 4).shape == (33, 65, 0)
    with pytest.raises(ValueError, match="^All quantiles must be >= 0 and <= 1$"):
        gridpp.neighbourhood_quantiles_fast(f, [0.5, 1.5], 4, [1.0, 2.0])
