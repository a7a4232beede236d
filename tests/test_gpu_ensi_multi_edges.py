"""optimal_interpolation_ensi_multi_{ebe, ebesc, utem} at the hand-off between k_ensi_multi and k_ensi_multi_huge, at their limits
(64 / 65 selected observations, 64 / 65 valid members, 8192 candidates, 4096 members), at their clamps, grid-stride loops, tiny and
degenerate ensembles, error returns and input plumbing.  The cases, their references and the conditions that keep them from being
vacuous live in tests/ensi_multi_cases.py (checked without a GPU by tests/test_ensi_multi_edges_oracle.py); every comparison is
ensi_multi_golden.compare: the oracle's NaN pattern and |out - ref| / max(|ref|, 1e-2) < 1e-5 on every value."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import ensi_multi_cases as K
from tests import ensi_multi_golden as G
from tests.test_gpu_ensi_multi_parity import _run

pytestmark = pytest.mark.gpu
BUDGET = "GPP_OI_HUGE_BUDGET_MB"     # scratch budget of k_ensi_multi_huge: decides how many workgroups share the huge grid points


def run(name, grid_overload=False):
    return _run(K.case(name), grid_overload)


def verified(name, out):
    """`out` against the reference of the named case, after the case's own non-vacuity condition"""
    K.assert_not_vacuous(name)
    G.compare(out, K.reference(name))
    return out


# a. The clamp of k_ensi_multi_huge (ebe, ebesc; utem with 80 members).  The utem, E 9, S 700 set is not a huge case (utem goes to the
#    general kernel beyond 8192 candidates or 64 members only): with max_points 12 it reaches the clamp of k_ensi_multi behind the radix
#    select of 12 of 700 candidates; the utem clamp of the general kernel with few members is case e.
@pytest.mark.parametrize("name", ["a_ebe", "a_ebesc", "a_utem80", "a_utem9"])
def test_clamp_beyond_the_lds_areas(name):
    verified(name, run(name))


# b. Both kernels in one call: k_ensi_multi finishes the grid points with at most 64 selected observations and lists the others;
#    with a 1 MB budget one workgroup (0.55 MB of scratch) walks the whole list, reusing its scratch from cell to cell.
@pytest.mark.parametrize("variant", ["ebe", "ebesc"])
def test_both_kernels_in_one_call(variant, monkeypatch):
    name = "b_" + variant
    out = verified(name, run(name))
    monkeypatch.setenv(BUDGET, "1")
    assert_array_equal(verified(name, run(name)), out)


# c. 63 / 64 / 65 selected observations: the last grid points of the LDS system and the first of the one in HBM (utem: no limit here)
@pytest.mark.parametrize("mp", [63, 64, 65])
@pytest.mark.parametrize("variant", K.VARIANTS)
def test_selected_observations_at_the_lds_limit(variant, mp):
    name = "c_%s_%d" % (variant, mp)
    verified(name, run(name))


# d. utem: 63 / 64 valid members in k_ensi_multi, 65 in k_ensi_multi_huge; 65 valid of 66 with a gap in validIdx
@pytest.mark.parametrize("name", ["d_63", "d_64", "d_65", "d_66gap"])
def test_utem_member_limit(name):
    out = verified(name, run(name))
    if name == "d_66gap":
        assert_array_equal(out[:, 3], K.case(name)["background"][:, 3])
        assert (out[:, 4] != K.case(name)["background"][:, 4]).all()


# e. More than 8192 candidates: every grid point goes to the general kernel (global-memory sort of 16384 keys); 7 workgroups for 12
#    grid points under a 1 MB budget (0.13 MB of scratch each), 12 without
@pytest.mark.parametrize("name", ["e_utem_0", "e_utem_50", "e_ebe_50", "e_ebesc_50"])
def test_more_candidates_than_the_lds_sort_holds(name, monkeypatch):
    out = verified(name, run(name))
    monkeypatch.setenv(BUDGET, "1")
    assert_array_equal(verified(name, run(name)), out)


# f. Many members: xL of ebe ends in the last slot it may use (4096 members, 64 observations), the same in HBM (65 observations),
#    k += 256 loops over the members, rows of Y staged 63 at a time (utem, 260 members: chunk = 16384 / 260)
@pytest.mark.parametrize("name", ["f_ebe_4096_64", "f_ebe_4096_65", "f_ebesc_4097", "f_utem_260"])
def test_many_members(name):
    verified(name, run(name))


def test_ebe_refuses_more_than_4096_members():
    with pytest.raises(RuntimeError, match="4096"):
        run("f_ebe_4097")


# g. More grid points than the 2048 workgroups of k_ensi_multi
@pytest.mark.parametrize("grid_overload", [False, True])
@pytest.mark.parametrize("variant", K.VARIANTS)
def test_more_grid_points_than_workgroups(variant, grid_overload):
    verified("g_" + variant, run("g_" + variant, grid_overload))


# h. One, two and three members: 1 / sqrt(nV - 1) is infinite at one member, the Jacobi is skipped
@pytest.mark.parametrize("E,allow", [(1, False), (2, False), (2, True), (3, False)])
@pytest.mark.parametrize("variant", K.VARIANTS)
def test_tiny_ensembles(variant, E, allow):
    name = "h_%s_%d_%d" % (variant, E, allow)
    out = verified(name, run(name))
    if E == 1 and variant != "ebesc":
        assert_array_equal(out, K.case(name)["background"])


# i. Spread at, just over and just under the 0.0013 floor: at observations, at grid points, in background itself
@pytest.mark.parametrize("variant", ["ebe", "utem"])
def test_spread_at_the_floor(variant):
    verified("i_" + variant, run("i_" + variant))


# j. Selection edges
@pytest.mark.parametrize("variant", ["ebesc", "utem"])
def test_grid_points_without_observations_keep_the_background(variant):
    name = "j_far_" + variant
    out = verified(name, run(name))
    assert_array_equal(out[K.FAR_CELLS], K.case(name)["background"][K.FAR_CELLS])


@pytest.mark.parametrize("variant", K.VARIANTS)
def test_observations_with_a_nan_deciding_value_are_dropped(variant):
    verified("j_nan_" + variant, run("j_nan_" + variant))


@pytest.mark.parametrize("grid_overload", [False, True])
@pytest.mark.parametrize("variant", ["ebesc", "utem"])
def test_cartesian_coordinates(variant, grid_overload):
    verified("j_cart_" + variant, run("j_cart_" + variant, grid_overload))


@pytest.mark.parametrize("name", ["j_strip_", "j_stripT_"])
@pytest.mark.parametrize("variant", ["ebesc", "utem"])
def test_both_axis_orders_of_the_observation_bins(variant, name):
    verified(name + variant, run(name + variant))


# k. Error returns (the host reads the error word after the kernels have finished) and the call after them
def _recovers(before):
    assert_array_equal(verified("c_ebesc_64", run("c_ebesc_64")), before)


@pytest.mark.parametrize("name", ["k_sing_lds", "k_sing_huge"])
def test_singular_system_raises_and_the_next_call_is_clean(name):
    from oracle import oracle as O
    with pytest.raises(O.OracleSingular):
        K.oracle(K.case(name))
    before = verified("c_ebesc_64", run("c_ebesc_64"))
    with pytest.raises(RuntimeError, match="singular"):
        run(name)
    _recovers(before)


def test_scratch_budget_too_small_raises_and_the_next_call_is_clean(monkeypatch):
    before = verified("c_ebesc_64", run("c_ebesc_64"))
    K.assert_not_vacuous("c_ebe_65")                      # (every grid point of it is a huge one)
    monkeypatch.setenv(BUDGET, "0")
    with pytest.raises(RuntimeError, match="scratch budget"):
        run("c_ebe_65")
    monkeypatch.delenv(BUDGET)
    _recovers(before)


# l. Repeats in one process: the selection is sorted on unique keys, so the arithmetic order is fixed and every repeat equals its
#    first result bit for bit whatever ran in between (the workspaces are kept from call to call)
def test_repeats_are_bit_identical_whatever_ran_in_between():
    first = {}
    for name in ["e_utem_0", "h_ebe_1_0", "b_ebesc", "c_ebe_65", "e_utem_0", "b_ebesc"]:
        out = run(name)
        if name in first:
            assert_array_equal(out, first[name])
        else:
            first[name] = verified(name, out)


# m. Plumbing
@pytest.mark.parametrize("name", ["c_ebe_64", "c_ebesc_64", "d_64"])
def test_float64_inputs_give_the_float32_bits(name):
    c = K.case(name)
    c64 = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in c.items()}
    assert c64["background"].dtype == np.float64
    assert_array_equal(_run(c64, False), verified(name, run(name)))


@pytest.mark.parametrize("name", ["c_ebe_64", "c_ebesc_64", "d_64"])
def test_device_tensors_give_a_device_tensor_with_the_same_bits(name):
    import torch
    import gridpp_amd as gridpp
    c = K.case(name)
    h, v, w, mp, allow = c["params"]
    variant = str(c["variant"])
    t = {k: torch.from_numpy(c[k].copy()).cuda() for k in ("bratios", "background", "background_corr", "pobs", "pratios", "pbackground", "pbackground_corr")}
    b, p = gridpp.Points(c["blat"], c["blon"]), gridpp.Points(c["plat"], c["plon"])
    st = gridpp.BarnesStructure(h, v, w)
    if variant == "ebesc":
        out = gridpp.optimal_interpolation_ensi_multi_ebesc(b, t["bratios"], t["background"], p, t["pobs"], t["pratios"], t["pbackground"], st, int(mp), bool(allow))
    else:
        fn = gridpp.optimal_interpolation_ensi_multi_ebe if variant == "ebe" else gridpp.optimal_interpolation_ensi_multi_utem
        out = fn(b, t["bratios"], t["background"], t["background_corr"], p, t["pobs"], t["pratios"], t["pbackground"], t["pbackground_corr"], st, int(mp), bool(allow))
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == c["background"].shape
    assert_array_equal(out.cpu().numpy(), verified(name, run(name)))


@pytest.mark.parametrize("variant", ["ebe", "ebesc"])
def test_grid_overload_of_the_mixed_case_equals_the_points_overload(variant):
    name = "b_" + variant
    assert_array_equal(run(name, True), verified(name, run(name)))
