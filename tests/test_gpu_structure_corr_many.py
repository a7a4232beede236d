"""corr / corr_background of one point against many in ONE launch (gpp_structure_corr_many, gpp_structure_corr_points) against
the scalar call pair by pair, bit for bit.

The scalar path (gpp_structure_corr) is unchanged and pinned against the oracle and the reference's known answers elsewhere; the
new kernel runs the same device function, so every comparison here is np.array_equal on the uint32 views -- no tolerance.  The
cases, the pool of second points and the conditions that keep a case from passing vacuously are tests/structure_corr_cases.py
(checked without a GPU in tests/test_structure_corr_cases_oracle.py); the conditions are checked again here on the values the
device's scalar path gives.  The list of n points, the Points of n and the Y x X Grid are the first n (Y * X) points of a case's
pool, so the pairwise values are computed once per case and shared."""
import functools

import numpy as np
import pytest

import gridpp_amd as gridpp
from tests import structure_corr_cases as K

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _p1(centre, variant):
    elev, laf = K.P1_VARIANTS[variant]
    return gridpp.Point(centre[0], centre[1], elev, laf)


@functools.lru_cache(maxsize=None)
def _case(index):
    """the structure of a case, and per first point: the pool, its Point objects and the scalar values {(variant, background): N floats}"""
    case = K.CASES[index]
    structure = case.build(gridpp)
    per_centre = []
    for centre in case.centres:
        lats, lons, elevs, lafs = K.pool(centre)
        points = [gridpp.Point(*q) for q in zip(lats, lons, elevs, lafs)]
        expected = {}
        for variant, background in K.COMBOS:
            p1 = _p1(centre, variant)
            scalar = structure.corr_background if background else structure.corr
            values = np.array([scalar(p1, q) for q in points], np.float32)
            values.setflags(write=False)
            why = K.vacuous(values, True, case.cv and background)
            assert why is None, (case, centre, variant, background, why)
            expected[variant, background] = values
        if case.cv:   # the two flags differ on a point closer than the cross-validation distance
            near = np.array([gridpp.KDTree.calc_straight_distance(points[0], q) <= 2000 for q in points])
            assert np.any(expected["full", 0][near] != expected["full", 1][near])
        per_centre.append((centre, (lats, lons, elevs, lafs), points, expected))
    return case, structure, per_centre


CASE_IDS = list(range(len(K.CASES)))
case_param = pytest.mark.parametrize("index", CASE_IDS, ids=[repr(c) for c in K.CASES])


@case_param
def test_list_of_points(index):
    case, structure, per_centre = _case(index)
    for centre, _, points, expected in per_centre:
        for (variant, background), values in expected.items():
            p1 = _p1(centre, variant)
            call = structure.corr_background if background else structure.corr
            for n in K.SIZES:
                for container in (list, tuple):
                    out = call(p1, container(points[:n]))
                    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (n,)
                    assert _same(out, values[:n]), (case, centre, variant, background, n)
                    if variant != "full" or background or n not in (0, 257):
                        break   # (tuples: one variant and two sizes are enough)


@case_param
def test_points_handle_host_and_device(index):
    import torch
    case, structure, per_centre = _case(index)
    for centre, (lats, lons, elevs, lafs), _, expected in per_centre:
        for n in K.SIZES:
            sets = [gridpp.Points(lats[:n], lons[:n], elevs[:n], lafs[:n])]
            if n == 257:   # a KDTree has neither elevations nor land-area fractions: the values of second points without them
                sets.append(gridpp.KDTree(lats[:n], lons[:n]))
            for to in sets:
                for (variant, background), values in expected.items():
                    p1 = _p1(centre, variant)
                    call = structure.corr_background if background else structure.corr
                    want = values[:n]
                    if isinstance(to, gridpp.KDTree):
                        scalar = structure._corr
                        want = np.array([scalar(p1, gridpp.Point(la, lo), background) for la, lo in zip(lats[:n], lons[:n])], np.float32)
                    host = call(p1, to)
                    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and host.shape == (n,)
                    assert _same(host, want), (case, centre, variant, background, n)
                    dev = call(p1, to, device="cuda")
                    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (n,)
                    assert _same(dev.cpu().numpy(), host), (case, centre, variant, background, n)


@case_param
def test_grid_handle_is_row_major(index):
    import torch
    case, structure, per_centre = _case(index)
    for centre, (lats, lons, elevs, lafs), _, expected in per_centre:
        for Y, X in K.GRIDS:
            n = Y * X
            grid = gridpp.Grid(*(a[:n].reshape(Y, X) for a in (lats, lons, elevs, lafs)))
            for (variant, background), values in expected.items():
                p1 = _p1(centre, variant)
                call = structure.corr_background if background else structure.corr
                host = call(p1, grid)
                assert isinstance(host, np.ndarray) and host.dtype == np.float32 and host.shape == (Y, X)
                assert _same(host, values[:n].reshape(Y, X)), (case, centre, variant, background, Y, X)   # cell (y, x) is point y * X + x
                dev = call(p1, grid, device=torch.device("cuda", 0))
                assert dev.is_cuda and tuple(dev.shape) == (Y, X) and _same(dev.cpu().numpy(), host)


def test_spatial_first_points_take_different_scales():
    """the three first points of the spatially varying case see three different scales: the lookup at the first point matters"""
    _, structure, per_centre = _case([repr(c) for c in K.CASES].index("spatial_barnes"))
    assert len({structure.localization_distance(_p1(centre, "full")) for centre, _, _, _ in per_centre}) == 3
    tables = [expected["full", 0] for _, _, _, expected in per_centre]
    assert not _same(tables[0], tables[1]) and not _same(tables[1], tables[2])


def test_other_second_arguments_stay_the_scalar_call():
    s = gridpp.BarnesStructure(K.H, K.V, K.W)
    p1, p2 = gridpp.Point(60, 10, 100, 0.5), gridpp.Point(60.03, 10.02, 150, 0.25)
    assert isinstance(s.corr(p1, p2), float) and 0 < s.corr(p1, p2) < 1
    assert s.corr(p1, [p2])[0] == np.float32(s.corr(p1, p2)) == s.corr(p1, gridpp.Points([60.03], [10.02], [150], [0.25]))[0]
    assert s.corr(p1, p2, device="cuda") == s.corr(p1, p2)          # the keyword only matters for a Points / KDTree / Grid
    with pytest.raises(ValueError):
        s.corr(p1, gridpp.Points([60.03], [10.02]), device="cpu")
