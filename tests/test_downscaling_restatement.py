"""CPU: the float32 composition of tests/downscaling_ref.py, built on the oracle's nearest / bilinear, reproduces every known
answer of the reference's tests/test_downscaling.py, test_simple_gradient.py and test_full_gradient.py
(tests/golden/downscaling_known_answers.json).  This pins the checker that the GPU tests hold the fused kernel to."""
import numpy as np
import pytest

from tests import downscaling_ref as R

CASES = [c for c in R.known_answers() if "expected" in c]


def compose_oracle(c):
    from oracle import oracle as O
    glats, glons, gelevs, glafs = R.set_arrays(c["igrid"])
    qlats, qlons, qelevs, qlafs = R.set_arrays(c["output"])
    d = R.oracle_downscaler(O, glats, glons, qlats, qlons, c["downscaler"])
    values = np.asarray(c["values"], np.float32)
    nq = np.size(qlats)
    oelevs = np.full(nq, np.nan) if qelevs is None else qelevs
    olafs = np.full(nq, np.nan) if qlafs is None else qlafs
    if c["function"] == "downscaling":
        out = d(values)
    elif c["function"] == "simple_gradient":
        out = R.compose_simple(d, values, gelevs, oelevs, c["elev_gradient"])
    else:
        out = R.compose_full(d, values, R.present(c.get("elev_gradient")), R.present(c.get("laf_gradient")), gelevs, glafs, oelevs, olafs)
    lead = values.shape[:-2]
    return out.reshape(lead + np.shape(qlats)) if c["output"]["type"] == "grid" else out.reshape(lead + (nq,))


def test_known_answers_cover_the_three_reference_files():
    srcs = {c["source"].split(":")[0] for c in R.known_answers()}
    assert srcs == {"tests/test_downscaling.py", "tests/test_simple_gradient.py", "tests/test_full_gradient.py"}
    assert len(CASES) >= 40


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_composition_reproduces_known_answer(case):
    out = compose_oracle(case)
    expected = np.asarray(case["expected"], np.float64)
    assert out.shape == expected.shape
    if case["exact"]:
        np.testing.assert_array_equal(out, expected)
    else:
        np.testing.assert_array_almost_equal(out, expected)


def test_composition_distinguishes_the_terms():
    """the checker is not vacuous: dropping a term, or the validity test of full_gradient, changes known answers"""
    c = next(x for x in CASES if x["id"] == "full_grid_to_grid_all_2d")
    dropped = dict(c, laf_gradient=[])
    assert not np.array_equal(compose_oracle(dropped), np.asarray(c["expected"], np.float64))
    s = next(x for x in CASES if x["id"] == "simple_no_grid_elev_0")
    assert np.all(np.isnan(compose_oracle(s)))   # simple_gradient has no validity test: NaN elevation -> NaN even at gradient 0
