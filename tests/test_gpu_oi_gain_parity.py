"""The reusable OI gain (gridpp_amd.optimal_interpolation_gain) against the CPU oracle on seeded inputs: every field a gain analyses
equals the oracle's optimal_interpolation of that field alone, with the measure of tests/test_gpu_oi_parity.py (|out - ref| /
max(|ref|, 1e-3) < 1e-5, equal NaN patterns, no cell left out).  Selections and weights are also pinned directly, the weights as
|dw| <= 1e-5 max|w| per cell against numpy.linalg.solve on the double matrix of the oracle's correlations.

gpp_oi_gain_apply has two kernels: a cell per lane below 16 fields, a field per lane from 16 fields on (and a second pass of the lanes
beyond 64 fields).  The stacks below hold 1, 3, 15 fields (the first), 16, 17 and 70 fields (the second)."""
import numpy as np
import pytest

from tests.test_gpu_oi_parity import RTOL, check, make_case, rel_err

pytestmark = pytest.mark.gpu


def handles(c, gridpp=None):
    """(Grid, Points) of the library and the oracle's point sets of a make_case dictionary"""
    from oracle import oracle as O
    if gridpp is None:
        import gridpp_amd as gridpp
    e = (c["gelev"], c["glaf"]) if c["gelev"] is not None else ((), ())
    pe = (c["pelev"], c["plaf"]) if c["pelev"] is not None else ((), ())
    grid = gridpp.Grid(c["lats"], c["lons"], e[0], e[1], c["ctype"])
    points = gridpp.Points(c["plat"], c["plon"], pe[0], pe[1], c["ctype"])
    og = O.Pts(c["lats"].ravel(), c["lons"].ravel(), None if c["gelev"] is None else c["gelev"].ravel(),
               None if c["glaf"] is None else c["glaf"].ravel(), c["ctype"])
    op = O.Pts(c["plat"], c["plon"], c["pelev"], c["plaf"], c["ctype"])
    return grid, points, og, op


def stack(seed, shape, S, E):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, shape + (E,)).astype(np.float32), rng.normal(0, 1, (S, E)).astype(np.float32),
            rng.normal(0, 1, (S, E)).astype(np.float32))


def check_stack(out, bg, pobs, pbg, og, op, ratios, ost, mp, allow=True):
    """every field of the stack against the oracle's analysis of that field alone"""
    from oracle import oracle as O
    assert out.shape == bg.shape and out.dtype == np.float32
    E = bg.shape[-1]
    for e in range(E):
        ob = pobs if pobs.ndim == 1 else pobs[:, e]
        ref = O.oi(og, bg[..., e].ravel(), op, ob, ratios, pbg[:, e], ost, mp, allow).reshape(bg.shape[:-1])
        check(np.ascontiguousarray(out[..., e]), ref)


@pytest.fixture(scope="module")
def odd_case():
    """37 x 53 grid, 150 stations, BarnesStructure(12000), max_points 12: one gain for all the stacks"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = make_case(5, 37, 53, 150)
    grid, points, og, op = handles(c)
    gain = gridpp.optimal_interpolation_gain(grid, points, c["ratios"], gridpp.BarnesStructure(12000), 12)
    return c, gain, og, op, O.Barnes(12000)


def test_one_field_is_optimal_interpolation(odd_case):
    from oracle import oracle as O
    c, gain, og, op, ost = odd_case
    out = gain.apply(c["bg"], c["obs"], c["pbg"])
    ref = O.oi(og, c["bg"].ravel(), op, c["obs"], c["ratios"], c["pbg"], ost, 12).reshape(37, 53)
    check(out, ref)
    assert np.abs(out - c["bg"]).max() > 0.1
    assert gain.max_points == 12 and gain.counts().max() == 12 == gain.largest_selection
    assert gain.nbytes >= 37 * 53 * 12 * 12


@pytest.mark.parametrize("E", [3, 15, 16, 17, 70])
@pytest.mark.parametrize("pobs_per_field", [False, True])
def test_field_stacks(odd_case, E, pobs_per_field):
    c, gain, og, op, ost = odd_case
    bg, pobs, pbg = stack(100 + E, (37, 53), 150, E)
    if not pobs_per_field:
        pobs = c["obs"]
    out = gain.apply(bg, pobs, pbg)
    check_stack(out, bg, pobs, pbg, og, op, c["ratios"], ost, 12)


@pytest.mark.parametrize("E", [1, 20])
def test_points_background_with_a_partial_last_tile(E):
    """1000 shuffled points: tiles of 64 consecutive points without spatial coherence, the last one holds 40"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = make_case(5, 37, 53, 150)
    rng = np.random.default_rng(3)
    n = 1000
    blat, blon = rng.random(n), rng.random(n)
    bpoints, points = gridpp.Points(blat, blon), gridpp.Points(c["plat"], c["plon"])
    gain = gridpp.optimal_interpolation_gain(bpoints, points, c["ratios"], gridpp.BarnesStructure(12000), 12)
    og, op = O.Pts(blat, blon), O.Pts(c["plat"], c["plon"])
    bg, pobs, pbg = stack(7, (n,), 150, E)
    if E == 1:
        out = gain.apply(bg[:, 0], pobs[:, 0], pbg[:, 0])
        assert out.shape == (n,)
        out = out[:, None]
    else:
        out = gain.apply(bg, pobs, pbg)
    check_stack(out, bg, pobs, pbg, og, op, c["ratios"], O.Barnes(12000), 12)
    assert gain.counts().shape == (n,) and gain.indices().shape == (n, 12)


@pytest.mark.parametrize("max_points", [1, 30, 33, 62])
def test_max_points_both_tile_sizes_with_elevation_and_laf(max_points):
    """1 .. 32 build on the 32-slot lists, 33 .. 62 on the 62-slot lists"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = make_case(11, 48, 48, 300, with_elev=True)
    grid, points, og, op = handles(c)
    gain = gridpp.optimal_interpolation_gain(grid, points, c["ratios"], gridpp.BarnesStructure(10000, 200, 0.5), max_points)
    out = gain.apply(c["bg"], c["obs"], c["pbg"])
    ref = O.oi(og, c["bg"].ravel(), op, c["obs"], c["ratios"], c["pbg"], O.Barnes(10000, 200, 0.5), max_points).reshape(48, 48)
    check(out, ref)
    bg, pobs, pbg = stack(12, (48, 48), 300, 16)
    check_stack(gain.apply(bg, pobs, pbg), bg, pobs, pbg, og, op, c["ratios"], O.Barnes(10000, 200, 0.5), max_points)
    assert gain.counts().max() <= max_points


SEL_SEED, SEL_H, SEL_MP = 23, 2500.0, 5


def test_selections_and_weights_pinned_directly():
    """40 x 56 Cartesian grid with two coincident stations, h = 2500 (localization 9.1 km: some corner has no station in range), max_points 5.
    counts() equals the oracle's number of selected observations at EVERY cell; at 40 cells spread over the grid indices() equals
    O.oi_selection as a set (no chosen cell straddles a tie: checked on the CPU for this seed, and asserted) and weights() equals
    numpy.linalg.solve((P + R)^T, g) in double on the oracle's correlations."""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = make_case(SEL_SEED, 40, 56, 250, geodetic=False, dup=True)
    grid, points, og, op = handles(c)
    ost = O.Barnes(SEL_H)
    gain = gridpp.optimal_interpolation_gain(grid, points, c["ratios"], gridpp.BarnesStructure(SEL_H), SEL_MP)
    counts, indices, weights = gain.counts().ravel(), gain.indices().reshape(-1, SEL_MP), gain.weights().reshape(-1, SEL_MP)
    assert counts.dtype == np.int32 and indices.dtype == np.int32 and weights.dtype == np.float64
    ones = np.ones(250, np.float32)
    ref_counts = np.array([O.oi_selection(og, cell, op, ones, ones, ost, SEL_MP)[0].size for cell in range(40 * 56)])
    np.testing.assert_array_equal(counts, ref_counts)
    corners = [0, 55, 39 * 56, 39 * 56 + 55]
    assert any(counts[k] == 0 for k in corners) and (counts == SEL_MP).any()
    for cell in range(40 * 56):   # padding behind the selection
        assert (indices[cell, counts[cell]:] == -1).all() and (weights[cell, counts[cell]:] == 0).all()
    pt = lambda P, i: (P.x[i], P.y[i], P.z[i], P.elevs[i], P.lafs[i])
    chosen = list(range(3, 40 * 56, 57))[:38] + [0, 39 * 56 + 55]   # (the two corners without a station in range among them)
    assert len(chosen) == 40 and counts[0] == 0 == counts[39 * 56 + 55]
    for cell in chosen:
        sel, tie = O.oi_selection(og, cell, op, ones, ones, ost, SEL_MP)
        assert not tie
        n = counts[cell]
        got = indices[cell, :n]
        assert (np.diff(got) > 0).all() and set(got.tolist()) == set(sel.tolist())
        if n == 0:
            continue
        A = np.array([[ost.corr(pt(op, i), pt(op, j)) for j in got] for i in got], np.float64) + np.diag(c["ratios"][got].astype(np.float64))
        g = np.array([ost.corr(pt(og, cell), pt(op, j)) for j in got], np.float64)
        w = np.linalg.solve(A.T, g)
        assert np.max(np.abs(weights[cell, :n] - w)) <= 1e-5 * np.max(np.abs(w)), cell
    # the coincident pair (stations 0 and 1) is selected together somewhere on the grid, and the analysis there is the oracle's
    both = [(0 in indices[k, :counts[k]]) and (1 in indices[k, :counts[k]]) for k in range(40 * 56)]
    assert any(both)
    out = gain.apply(c["bg"], c["obs"], c["pbg"])
    check(out, O.oi(og, c["bg"].ravel(), op, c["obs"], c["ratios"], c["pbg"], ost, SEL_MP).reshape(40, 56))


def test_usable_mask_and_invalid_values():
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = make_case(33, 30, 44, 160)
    grid, points, og, op = handles(c)
    rng = np.random.default_rng(9)
    usable = np.ones(160, bool)
    usable[rng.choice(160, 16, replace=False)] = False
    gain = gridpp.optimal_interpolation_gain(grid, points, c["ratios"], gridpp.BarnesStructure(11000), 10, usable=usable)
    bg, pobs, pbg = stack(34, (30, 44), 160, 3)
    masked = np.flatnonzero(~usable)
    pobs[masked[:8], :] = np.nan              # ignored: the stations are not usable
    pbg[masked[8:], 1] = np.nan
    bg[4, 5, 1] = np.nan                      # an invalid background passes through, in its field only
    bg[17, 40, 1] = np.inf
    out = gain.apply(bg, pobs, pbg)
    assert set(gain.indices()[gain.indices() >= 0].tolist()).isdisjoint(masked.tolist())
    for e in range(3):
        ob = pobs[:, e].copy()
        ob[masked] = np.nan                   # the oracle drops a station with an invalid observation (oi.cpp:252)
        pb = np.where(np.isnan(pbg[:, e]), 0, pbg[:, e]).astype(np.float32)
        ref = O.oi(og, bg[..., e].ravel(), op, ob, c["ratios"], pb, O.Barnes(11000), 10).reshape(30, 44)
        got = np.ascontiguousarray(out[..., e])
        fin = np.isfinite(bg[..., e])
        assert (np.isnan(got) == np.isnan(ref)).all() and (np.isinf(got) == np.isinf(bg[..., e])).all()
        assert rel_err(got[fin], ref[fin]) < RTOL
    assert np.isnan(out[4, 5, 1]) and np.isinf(out[17, 40, 1]) and np.isfinite(out[..., 0]).all() and np.isfinite(out[..., 2]).all()
    # an invalid value at a USABLE station: the lowest (field, station) is named
    s1, s2 = np.flatnonzero(usable)[[20, 90]]
    bad = pbg.copy()
    bad[s2, 2] = np.nan
    bad[s1, 2] = np.nan
    with pytest.raises(ValueError, match=r"usable station %d of field 2\b" % s1):
        gain.apply(bg, pobs, bad)
    bad_obs = pobs.copy()
    bad_obs[s2, 2] = np.inf
    with pytest.raises(ValueError, match=r"usable station %d of field 2\b" % s2):
        gain.apply(bg, bad_obs, pbg)
    # no usable station at all, and no station at all: valid gains without selections
    none = gridpp.optimal_interpolation_gain(grid, points, c["ratios"], gridpp.BarnesStructure(11000), 10, usable=np.zeros(160, bool))
    assert (none.counts() == 0).all()
    np.testing.assert_array_equal(none.apply(c["bg"], c["obs"], c["pbg"]), c["bg"])
    empty = gridpp.optimal_interpolation_gain(grid, gridpp.Points(), [], gridpp.BarnesStructure(11000), 10)
    np.testing.assert_array_equal(empty.apply(c["bg"], [], []), c["bg"])


@pytest.mark.parametrize("E", [2, 16])
def test_no_extrapolation_clamps_per_field(E):
    """innovations of opposite sign in neighbouring fields: the clamp of oi.cpp:318-334 takes the extremes of ITS field"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = make_case(21, 40, 56, 250, geodetic=False, dup=True)
    grid, points, og, op = handles(c)
    gain = gridpp.optimal_interpolation_gain(grid, points, c["ratios"], gridpp.BarnesStructure(9000), 10)
    bg, pobs, pbg = stack(22, (40, 56), 250, E)
    sign = np.where(np.arange(E) % 2 == 0, 1.0, -1.0).astype(np.float32)
    pobs = (pbg + sign * np.abs(pobs) - 0.2 * sign).astype(np.float32)   # mostly one sign per field, a few of the other
    out = gain.apply(bg, pobs, pbg, False)
    check_stack(out, bg, pobs, pbg, og, op, c["ratios"], O.Barnes(9000), 10, allow=False)
    free = gain.apply(bg, pobs, pbg, True)
    assert (free != out).any()                # the clamp was at work


def test_analysis_variance():
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = make_case(31, 48, 40, 200)
    grid, points, og, op = handles(c)
    rng = np.random.default_rng(7)
    bvar = rng.uniform(0.5, 2, (48, 40)).astype(np.float32)
    bvp = rng.uniform(0.5, 2, 200).astype(np.float32)
    ratios = (c["ratios"] / bvp).astype(np.float32)          # float32 division, as oi.cpp:194
    gain = gridpp.optimal_interpolation_gain(grid, points, ratios, gridpp.BarnesStructure(10000), 16)
    ref, rvar = O.oi_full(og, c["bg"].ravel(), bvar.ravel(), op, c["obs"], c["ratios"], c["pbg"], bvp, O.Barnes(10000), 16)
    check(gain.apply(c["bg"], c["obs"], c["pbg"]), ref.reshape(48, 40))
    check(gain.analysis_variance(bvar), rvar.reshape(48, 40))


def _generic_case(c, st, ost, mp, cell_params=None, obs_params=None):
    import gridpp_amd as gridpp
    from oracle import oracle as O
    grid, points, og, op = handles(c)
    Y, X = c["bg"].shape
    ones_g, ones_p = np.ones((Y, X), np.float32), np.ones(c["obs"].size, np.float32)
    gain = gridpp.optimal_interpolation_gain(grid, points, c["ratios"], st(gridpp, grid), mp)
    ref, rvar = O.oi_full_generic(og, c["bg"].ravel(), ones_g.ravel(), op, c["obs"], c["ratios"], c["pbg"], ones_p, ost(O), mp, True,
                                  cell_params(og, op)[0] if cell_params else None, cell_params(og, op)[1] if cell_params else None)
    out = gain.apply(c["bg"], c["obs"], c["pbg"])
    check(out, ref.reshape(Y, X))
    check(gain.analysis_variance(ones_g), rvar.reshape(Y, X))
    assert np.abs(out - c["bg"]).max() > 0.05


def test_cressman_structure_with_signed_vertical_factors():
    """Cressman factors on signed elevation / laf differences: P is not symmetric"""
    c = make_case(61, 40, 36, 120, with_elev=True)
    _generic_case(c, lambda g, grid: g.CressmanStructure(30000, 300, 0.6), lambda O: O.Struct("Cressman", 30000, 300, 0.6), 12)


def test_multiple_structure():
    c = make_case(62, 36, 40, 150, with_elev=True)
    _generic_case(c, lambda g, grid: g.MultipleStructure(g.BarnesStructure(12000), g.LinearStructure(0, 0.2, 0), g.PowerlawStructure(1, 1, 0.7)),
                  lambda O: O.Struct.multiple(O.Struct("Barnes", 12000), O.Struct("Linear", 0, 0.2, 0), O.Struct("Powerlaw", 1, 1, 0.7)), 14)


def test_cross_validation_over_barnes():
    c = make_case(62, 36, 40, 150, with_elev=True)
    _generic_case(c, lambda g, grid: g.CrossValidation(g.BarnesStructure(12000, 200, 0.5), 3000),
                  lambda O: O.Struct("Barnes", 12000, 200, 0.5).cross_validation(3000), 14)


def test_spatially_varying_barnes():
    """h within 20 % of 9000 per grid point: corr(p1, p2) takes p1's scales, P is not symmetric"""
    from oracle import oracle as O
    c = make_case(90, 30, 34, 100, with_elev=True)
    rng = np.random.default_rng(5)
    hf = (9000 * rng.uniform(0.8, 1.2, (30, 34))).astype(np.float32)
    vf = np.full((30, 34), 300, np.float32)
    wf = np.full((30, 34), 0.6, np.float32)
    min_rho = 0.0013

    def params(og, op):
        ci, oi = np.arange(og.n), O.nearest_indices(og, op)
        Rf = np.array([O.structure_localization("Barnes", h, min_rho) for h in hf.ravel()], np.float32)
        return [a.ravel()[ci] for a in (hf, vf, wf)] + [Rf[ci]], [a.ravel()[oi] for a in (hf, vf, wf)] + [Rf[oi]]
    _generic_case(c, lambda g, grid: g.BarnesStructure(grid, hf, vf, wf, min_rho), lambda O_: O_.Struct("Barnes", 9000), 10, params)


def test_singular_system_raises_like_optimal_interpolation():
    """two coincident stations with ratio 0 and nothing else: P + R = [[1, 1], [1, 1]] at every cell in range"""
    import gridpp_amd as gridpp
    lats, lons = np.meshgrid(np.linspace(0, 1, 8), np.linspace(0, 1, 8), indexing="ij")
    grid = gridpp.Grid(lats, lons)
    points = gridpp.Points([0.5, 0.5], [0.5, 0.5])
    bg = np.zeros((8, 8), np.float32)
    ratios = np.zeros(2, np.float32)
    st = gridpp.BarnesStructure(50000)
    with pytest.raises(RuntimeError, match="singular"):
        gridpp.optimal_interpolation(grid, bg, points, [1.0, 1.0], ratios, [0.0, 0.0], st, 5)
    with pytest.raises(RuntimeError, match="singular"):
        gridpp.optimal_interpolation_gain(grid, points, ratios, st, 5)
    # the same stations with a positive ratio are fine
    gain = gridpp.optimal_interpolation_gain(grid, points, ratios + 0.5, st, 5)
    assert gain.counts().max() == 2


def test_state_lifetime_and_device_tensors():
    import torch
    import gridpp_amd as gridpp
    c = make_case(5, 37, 53, 150)
    grid, points, og, op = handles(c)
    st = gridpp.BarnesStructure(12000)
    gain = gridpp.optimal_interpolation_gain(grid, points, c["ratios"], st, 12)
    bg, pobs, pbg = stack(41, (37, 53), 150, 17)
    first, one = gain.apply(bg, pobs, pbg), gain.apply(c["bg"], c["obs"], c["pbg"])
    np.testing.assert_array_equal(gain.apply(bg, pobs, pbg).view(np.uint32), first.view(np.uint32))
    # an optimal_interpolation call on another geometry in between
    c2 = make_case(11, 48, 48, 300, with_elev=True)
    g2, p2, _, _ = handles(c2)
    gridpp.optimal_interpolation(g2, c2["bg"], p2, c2["obs"], c2["ratios"], c2["pbg"], gridpp.BarnesStructure(10000, 200, 0.5), 15)
    np.testing.assert_array_equal(gain.apply(bg, pobs, pbg).view(np.uint32), first.view(np.uint32))
    # what the gain was built from is gone
    del grid, points, st, g2, p2
    import gc
    gc.collect()
    np.testing.assert_array_equal(gain.apply(bg, pobs, pbg).view(np.uint32), first.view(np.uint32))
    np.testing.assert_array_equal(gain.apply(c["bg"], c["obs"], c["pbg"]).view(np.uint32), one.view(np.uint32))
    # torch CUDA tensors in, a torch CUDA tensor out, the same bits
    dev = [torch.from_numpy(a).cuda() for a in (bg, pobs, pbg)]
    out = gain.apply(*dev)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), first.view(np.uint32))
    var = gain.analysis_variance(torch.ones(37, 53, device="cuda"))
    assert var.is_cuda and float(var.max()) <= 1.0
    with pytest.raises(ValueError, match="either all field arguments"):
        gain.apply(dev[0], pobs, pbg)
    nbytes = gain.nbytes
    assert nbytes >= 37 * 53 * 12 * 12
    gain.release()
    with pytest.raises(RuntimeError, match="released"):
        gain.apply(bg, pobs, pbg)
