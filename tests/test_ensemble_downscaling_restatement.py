"""CPU: the numpy float32 restatement of tests/ensemble_downscaling_ref.py, built on the oracle's nearest index, calc_statistic
and calc_quantile, reproduces every known answer of the reference's tests/test_downscale_probability.py and
tests/test_mask_threshold_downscale_consensus.py (tests/golden/ensemble_downscaling_known_answers.json) exactly.  This pins the
checker that the GPU tests hold the kernels to.  The reference has no test of `smart`: its restatement is pinned by nothing but
its own reading of src/api/smart.cpp (see tests/test_gpu_smart_parity.py)."""
import numpy as np
import pytest

from tests import ensemble_downscaling_ref as R

CASES = R.known_answers()


def nearest_idx():
    from oracle import oracle as O
    g = R.golden()["grids"]
    idx = O.nearest_indices(O.Pts(np.ravel(g["igrid"]["lats"]), np.ravel(g["igrid"]["lons"])),
                            O.Pts(np.ravel(g["ogrid"]["lats"]), np.ravel(g["ogrid"]["lons"])))
    return O, idx


def test_known_answers_cover_the_two_reference_files():
    srcs = [c["source"].split(":")[0] for c in CASES]
    assert srcs.count("tests/test_downscale_probability.py") == 4
    assert srcs.count("tests/test_mask_threshold_downscale_consensus.py") == 6
    assert len({c["id"] for c in CASES}) == 10


def test_nearest_indices_of_the_known_answer_grids():
    _, idx = nearest_idx()
    np.testing.assert_array_equal(idx, R.golden()["grids"]["nearest_indices"])


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_restatement_reproduces_known_answer(case):
    O, idx = nearest_idx()
    out = R.compose_case(O, case, idx)
    expected = np.asarray(case["expected"], np.float32)
    assert out.dtype == np.float32 and out.shape == expected.shape
    np.testing.assert_array_equal(out, expected)


def test_restatement_distinguishes_the_operators_and_the_validity_test():
    """the checker is not vacuous: Lt for Leq, or no validity test on threshold_values, changes known answers"""
    O, idx = nearest_idx()
    by_id = {c["id"]: c for c in CASES}
    for cid in ("probability_leq", "mask_leq_mean"):
        c = by_id[cid]
        assert not np.array_equal(R.compose_case(O, c, idx, op=R.Lt), np.asarray(c["expected"], np.float32))
    c = by_id["mask_geq_count_nan_threshold_value"]
    assert not np.array_equal(R.compose_case(O, c, idx, check_valid=False), np.asarray(c["expected"], np.float32))
