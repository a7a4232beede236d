"""The cases of tests/bilinear_cases.py on the CPU: they reach every branch and both roots of the general-quadrilateral solve
(so tests/test_gpu_bilinear_general.py cannot silently degrade into the parallelogram formula), and the oracle -- the side the
device is compared with -- agrees with a float64 Newton inversion of the same boxes.

Three of the 24 cases make the oracle raise OracleDistorted for every query inside the mesh: REFERENCE_THROWS below."""
import numpy as np
import pytest

from tests import bilinear_cases as B

# The qa == 0 branch of the reference has no second root: its retry repeats the first one (src/api/bilinear.cpp:250-252; the
# other two branches retry with `- sqrt`).  On these orientations of the trapezoids the first root is the wrong one for every
# location inside the mesh (s = +-inf, t = 9 or -23), so the reference throws "Problem with bilinear interpolation" there, and so
# do the oracle and the device.  Their boxes still count for the coverage conditions and are searched like any other; the values
# are compared on the 21 other cases.
REFERENCE_THROWS = ("trapezoid0-flipY", "trapezoid0-flipX", "trapezoid1-transposed")
VALUE_CASES = [c for c in B.CASE_IDS if c not in REFERENCE_THROWS]

# max |oracle - truth| over the inside queries, field N(0, 3) (range 15 ... 23), measured per family on the case list of
# bilinear_cases.CASE_IDS (x86-64, glibc 2.39): metres 7.79e-6 (offset (0, 0); 9.1e-7 and 1.13e-6 at the two large offsets, where
# the float32 coordinates are multiples of 1/16 m and 1/2 m and every difference of the solve is exact), degrees 1.42e-5,
# trapezoid 8.55e-7.  What remains is the float32 rounding of the coordinate differences (half an ulp of a coordinate against
# one cell side) and of (s, t) themselves.  The tests allow 4 x these: another seed or another libm, not the kernel.
E_ORACLE = {"metres": 7.79e-6, "degrees": 1.42e-5, "trapezoid": 8.55e-7}
MARGIN = 4


def _inside(c):
    return c.boxes[:, 0] != 0


def oracle_raises(c):
    from oracle import oracle as O
    try:
        c.oracle_values
    except O.OracleDistorted:
        return True
    return False


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", B.CASE_IDS)
def test_no_box_takes_the_parallelogram_formula(cid):
    c = B.case(cid)
    cl = B.classify(c.lats, c.lons)
    assert cl["parallelogram"] == 0 and cl["both"] + cl["qb0"] + cl["qa0"] == cl["boxes"] == (c.shape[0] - 1) * (c.shape[1] - 1), cl


def test_every_branch_owns_all_boxes_of_two_cases():
    owned = {k: [] for k in ("both", "qb0", "qa0")}
    for cid in B.CASE_IDS:
        c = B.case(cid)
        cl = B.classify(c.lats, c.lons)
        for k in owned:
            if cl[k] == cl["boxes"]:
                owned[k].append(cid)
    for k, ids in owned.items():
        assert len(ids) >= 2, (k, ids)
        assert any(i in VALUE_CASES for i in ids), (k, ids)      # ... and of at least one case whose values are compared


def test_each_root_is_taken_by_a_thousand_inside_queries():
    first = second = 0
    for cid in VALUE_CASES:
        alpha_first, beta_first, has_alpha, has_beta = B.case(cid).roots
        first += int(np.sum(alpha_first & has_alpha))
        second += int(np.sum(~alpha_first & has_alpha))
    assert first >= 1000 and second >= 1000, (first, second)
    # flipping the metre mesh either way switches the root (both unknowns)
    a, b, _, _ = B.case("metres-asis").roots
    assert a.all() and b.all()
    for how in ("flipY", "flipX"):
        a, b, _, _ = B.case("metres-" + how).roots
        assert not a.any() and not b.any()


@pytest.mark.parametrize("cid", VALUE_CASES)
def test_the_case_interpolates(cid):
    c = B.case(cid)
    assert np.mean(c.oracle_values != c.nearest) >= 0.40


@pytest.mark.parametrize("cid", [c for c in VALUE_CASES if B.family(c) != "trapezoid"])
def test_warped_cases_reach_the_snap(cid):
    """nodes and edge midpoints: the float64 (u, v) lies outside [0, 1] by more than 1e-9, inside by the float box test"""
    _, u, v = B.case(cid).truth_values
    out = (u < -1e-9) | (u > 1 + 1e-9) | (v < -1e-9) | (v > 1 + 1e-9)
    assert int(np.sum(out)) >= 20


# ---- the oracle's behaviour ---------------------------------------------------------------------------------------------------------
def test_oracle_raises_only_where_the_reference_has_no_second_root():
    raising = [cid for cid in B.CASE_IDS if oracle_raises(B.case(cid))]
    assert tuple(raising) == REFERENCE_THROWS
    for cid in REFERENCE_THROWS:
        c = B.case(cid)
        cl = B.classify(c.lats, c.lons)
        assert cl["qa0"] == cl["boxes"]
        _, beta_first, has_alpha, has_beta = c.roots
        assert has_beta.all() and not has_alpha.any() and not beta_first.any()      # the one root this branch tries is out of range
        assert _inside(c).sum() > 2000


@pytest.mark.parametrize("cid", VALUE_CASES)
def test_oracle_against_float64_newton(cid):
    c = B.case(cid)
    m = _inside(c)
    tv = c.truth_values[0]
    assert np.isfinite(tv[m]).all() and np.isnan(tv[~m]).all()
    np.testing.assert_array_equal(c.oracle_values[~m], c.nearest[~m])
    err = float(np.max(np.abs(c.oracle_values[m] - tv[m])))
    print("%s: max |oracle - truth| = %.3g (recorded family maximum %.3g)" % (cid, err, E_ORACLE[c.family]))
    assert err <= MARGIN * E_ORACLE[c.family]


@pytest.mark.parametrize("cid", VALUE_CASES)
def test_oracle_reproduces_a_linear_field(cid):
    c = B.case(cid)
    m = _inside(c)
    _, u, v = c.truth_values
    assert float(np.max(np.abs(c.oracle_linear[m] - c.truth_linear[m]))) <= MARGIN * E_ORACLE[c.family]
    # against the closed form where the location is inside its box in float64 as well (a snapped one is clamped onto the box)
    strict = m & (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)
    assert strict.sum() > 1500
    assert float(np.max(np.abs(c.oracle_linear[strict] - c.lin(c.qlat, c.qlon)[strict]))) <= MARGIN * E_ORACLE[c.family]


# ---- grids of height or width 1 or 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", B.DEGENERATE_SHAPES)
def test_degenerate_shapes(shape):
    d = B.degenerate(shape)
    if min(shape) == 1:
        assert not d["boxes"][:, 0].any()
        np.testing.assert_array_equal(d["expected"], d["nearest"])
    else:
        assert d["boxes"][:, 0].tolist() == [1, 1, 1, 1, 0]
        assert d["expected"][1] != d["nearest"][1] and d["expected"][2] != d["nearest"][2]       # interior point, centre
        np.testing.assert_array_equal(d["expected"][[0, 3, 4]], d["nearest"][[0, 3, 4]])      # node, far corner, outside
        tv = B.truth(d["lats"], d["lons"], d["values"], d["boxes"], d["qlat"], d["qlon"])[0]
        np.testing.assert_allclose(d["expected"][:4], tv[:4], rtol=0, atol=4 * 2.0 ** -23 * float(d["values"].max()))
