"""Case builder of the optimal_interpolation_ensi_multi edge suites (tests/test_gpu_ensi_multi_edges.py on the GPU,
tests/test_ensi_multi_edges_oracle.py on the CPU): random cases in the dict layout that `_run` of test_gpu_ensi_multi_parity.py takes,
the named cases a .. k of the edge suite, and their references (the C oracle; the numpy + LAPACK restatement of
tools/make_ensi_multi_fixtures.py where the restatement accepts the case).

Every system is well conditioned: members are normal(0, 1), pratios lie in [0.1, 1] and bratios in [0.5, 1.5]."""
import functools
import os
import sys

import numpy as np

from tests.ensi_multi_golden import RTOL  # noqa: F401  (the one measure: ensi_multi_golden.compare)

F = np.float32
VARIANTS = ("ebe", "ebesc", "utem")
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UTEM260_FIXTURE = os.path.join(_ROOT, "tests", "golden", "ensi_multi_utem260.npz")


def make_case(variant, C, E, S, seed, h, max_points, allow, ctype=0, box=(1.0, 1.0), grid_shape=None, edit=None):
    """One random case.  Coordinates are uniform in a box of `box` degrees (lat, lon), or of box * 100 km in metres for ctype 1
    (Cartesian); `grid_shape` = (Y, X) with Y * X == C lets the case run through the Grid overload too; `edit(c, rng)` changes
    the arrays in place before anybody computes a reference."""
    rng = np.random.default_rng(seed)
    scale = 1e5 if ctype == 1 else 1.0
    blat, blon = (rng.random(C) * box[0] * scale).astype(F), (rng.random(C) * box[1] * scale).astype(F)
    plat, plon = (rng.random(S) * box[0] * scale).astype(F), (rng.random(S) * box[1] * scale).astype(F)
    bg, bgc = rng.normal(0, 1, (C, E)).astype(F), rng.normal(0, 1, (C, E)).astype(F)
    pbg, pbgc = rng.normal(0, 1, (S, E)).astype(F), rng.normal(0, 1, (S, E)).astype(F)
    pobs = rng.normal(0, 1, S).astype(F) if variant == "utem" else rng.normal(0, 1, (S, E)).astype(F)
    pr, br = rng.uniform(0.1, 1, S).astype(F), rng.uniform(0.5, 1.5, C).astype(F)
    Y, X = grid_shape if grid_shape else (0, C)
    assert Y == 0 or Y * X == C
    c = dict(variant=np.array(variant), shape=np.array([Y, X, E]), blat=blat, blon=blon, belev=np.full(C, np.nan, F), blaf=np.full(C, np.nan, F),
             bratios=br, background=bg, background_corr=bgc, plat=plat, plon=plon, pelev=np.full(S, np.nan, F), plaf=np.full(S, np.nan, F),
             pobs=pobs, pratios=pr, pbackground=pbg, pbackground_corr=pbgc, params=np.array([h, 0, 0, max_points, 1.0 if allow else 0.0]),
             ctype=np.array(ctype))
    if edit is not None:
        edit(c, rng)
    return c


def with_params(c, max_points=None, allow=None):
    """the same arrays with another max_points / allow_extrapolation"""
    d = dict(c)
    p = c["params"].copy()
    if max_points is not None:
        p[3] = max_points
    if allow is not None:
        p[4] = 1.0 if allow else 0.0
    d["params"] = p
    return d


def _oracle_sets(c):
    from oracle import oracle as O
    ct = int(c["ctype"])
    return O, O.Pts(c["blat"], c["blon"], ctype=ct), O.Pts(c["plat"], c["plon"], ctype=ct), O.Barnes(float(c["params"][0]))


def oracle(c):
    """the C oracle on a case (raises oracle.OracleSingular where arma::inv would throw)"""
    O, g, p, st = _oracle_sets(c)
    return O.oi_ensi_multi(str(c["variant"]), g, c["bratios"], c["background"], c["background_corr"], p, c["pobs"], c["pratios"],
                           c["pbackground"], c["pbackground_corr"], st, int(c["params"][3]), bool(c["params"][4]))


def restatement(c):
    """the independent numpy + LAPACK restatement (geodetic cases whose members are all valid)"""
    tools = os.path.join(_ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import make_ensi_fixtures as MF
    import make_ensi_multi_fixtures as MM
    h, v, w, mp, allow = c["params"]
    assert int(c["ctype"]) == 0 and MF._loc_readings_agree(float(h)), "the restatement does not take this case"
    with np.errstate(divide="ignore"):      # (one member: 1 / sqrt(nV - 1) is infinite in the reference too, and never used)
        return MM.ensi_multi(str(c["variant"]), c["blat"], c["blon"], c["belev"], c["blaf"], c["bratios"], c["background"], c["background_corr"],
                             c["plat"], c["plon"], c["pelev"], c["plaf"], c["pobs"], c["pratios"], c["pbackground"], c["pbackground_corr"],
                             float(h), float(v), float(w), int(mp), bool(allow))


def selection_counts(c):
    """(selected observations of every grid point, whether any has a rho tie at the max_points cut), by the oracle's own selection"""
    O, g, p, st = _oracle_sets(c)
    deciding = c["pobs"] if str(c["variant"]) == "utem" else np.ascontiguousarray(c["pobs"][:, 0])
    zeros = np.zeros(p.n, F)
    counts, tie = np.zeros(g.n, int), False
    for cell in range(g.n):
        sel, t = O.oi_selection(g, cell, p, deciding, zeros, st, int(c["params"][3]))
        counts[cell] = sel.size
        tie = tie or t
    return counts, tie


# ---- the edits of the named cases ------------------------------------------------------------------------------------------
def _density_gradient(c, rng):            # b: the first half of the observations crowd into a corner
    c["plat"][:130] *= F(0.4)
    c["plon"][:130] *= F(0.4)


def _member3_invalid(c, rng):             # d: one NaN at one observation takes member 3 out: validIdx has a gap
    c["pbackground_corr"][5, 3] = np.nan


FLOOR_OBS_CONST, FLOOR_OBS_ABOVE, FLOOR_OBS_BELOW = slice(0, 10), slice(10, 14), slice(14, 18)
FLOOR_CELLS_CORR, FLOOR_CELLS_BG = slice(0, 15), slice(10, 25)


def _spread_at_the_floor(c, rng):         # i: ensemble spread at, just above and just under the 0.0013 floor
    E = c["background"].shape[1]
    k = np.arange(E, dtype=F)
    c["pbackground_corr"][FLOOR_OBS_CONST] = c["pbackground_corr"][FLOOR_OBS_CONST, :1]
    c["pbackground_corr"][FLOOR_OBS_ABOVE] = c["pbackground_corr"][FLOOR_OBS_ABOVE, :1] + F(1e-3) * k     # std about 0.0017
    c["pbackground_corr"][FLOOR_OBS_BELOW] = c["pbackground_corr"][FLOOR_OBS_BELOW, :1] + F(7e-4) * k     # std about 0.0012
    c["background_corr"][FLOOR_CELLS_CORR] = c["background_corr"][FLOOR_CELLS_CORR, :1]
    c["background"][FLOOR_CELLS_BG] = c["background"][FLOOR_CELLS_BG, :1]


FAR_CELLS = slice(0, 8)
NAN_OBS = (1, 4, 7, 10, 13, 16)


def _cells_far_away(c, rng):              # j: nothing in range of the first 8 grid points
    c["blat"][FAR_CELLS] += F(5.0)


def _deciding_value_nan(c, rng):          # j: pobs[s, 0] (ebe / ebesc) or pobs[s] (utem) decides whether observation s is used
    if str(c["variant"]) == "utem":
        c["pobs"][list(NAN_OBS)] = np.nan
    else:
        c["pobs"][list(NAN_OBS), 0] = np.nan


def _two_obs_coincide(c, rng):            # k: observations 0 and 1 coincide and carry no error: two identical rows, an exact zero pivot
    c["plat"][1], c["plon"][1] = c["plat"][0], c["plon"][0]
    c["pratios"][:2] = 0


def _specs():
    s = {}
    # a. the clamp of k_ensi_multi_huge: the parameter sets of test_ensi_multi_beyond_the_lds_areas with allow = False (the fourth with
    #    max_points 12 so that the clamp bites)
    for name, (v, E, S, mp) in {"a_ebe": ("ebe", 10, 140, 100), "a_ebesc": ("ebesc", 10, 140, 0), "a_utem80": ("utem", 80, 120, 0),
                                "a_utem9": ("utem", 9, 700, 12)}.items():
        s[name] = dict(variant=v, C=10, E=E, S=S, seed=70 + E + S, h=200000, max_points=mp, allow=False)
    for v in VARIANTS:
        # b. both kernels in one call (ebe, ebesc); as a 10 x 20 grid for the plumbing test
        if v != "utem":
            s["b_" + v] = dict(variant=v, C=200, E=7, S=260, seed=11, h=12500, max_points=0, allow=False, grid_shape=(10, 20), edit=_density_gradient)
        # c. 63 / 64 / 65 selected observations
        for mp in (63, 64, 65):
            s["c_%s_%d" % (v, mp)] = dict(variant=v, C=12, E=5, S=150, seed=23, h=200000, max_points=mp, allow=False)
        # e. more than 8192 candidates (never max_points 0 for ebe / ebesc: an 8300 x 8300 LU)
        for mp in ((0, 50) if v == "utem" else (50,)):
            s["e_%s_%d" % (v, mp)] = dict(variant=v, C=12, E=5, S=8300, seed=31, h=400000, max_points=mp, allow=False)
        # g. more grid points than workgroups of k_ensi_multi; also a 46 x 50 grid
        s["g_" + v] = dict(variant=v, C=2300, E=4, S=50, seed=37, h=30000, max_points=6, allow=False, grid_shape=(46, 50))
        # h. one, two and three members
        for E, allow in ((1, False), (2, False), (2, True), (3, False)):
            s["h_%s_%d_%d" % (v, E, allow)] = dict(variant=v, C=40, E=E, S=30, seed=41, h=40000, max_points=0, allow=allow)
        # j. selection edges
        s["j_far_" + v] = dict(variant=v, C=30, E=5, S=20, seed=53, h=12500, max_points=0, allow=False, edit=_cells_far_away)
        s["j_nan_" + v] = dict(variant=v, C=30, E=5, S=20, seed=54, h=40000, max_points=0, allow=False, edit=_deciding_value_nan)
        s["j_cart_" + v] = dict(variant=v, C=30, E=5, S=20, seed=55, h=40000, max_points=8, allow=False, ctype=1, grid_shape=(5, 6))
        s["j_strip_" + v] = dict(variant=v, C=30, E=5, S=40, seed=56, h=12500, max_points=0, allow=False, box=(0.05, 2.0))
        s["j_stripT_" + v] = dict(variant=v, C=30, E=5, S=40, seed=56, h=12500, max_points=0, allow=False, box=(2.0, 0.05))
    # d. 63 / 64 / 65 valid members of utem, and 65 valid ones of 66 with a gap
    for E in (63, 64, 65):
        s["d_%d" % E] = dict(variant="utem", C=6, E=E, S=90, seed=29, h=200000, max_points=0, allow=False)
    s["d_66gap"] = dict(variant="utem", C=6, E=66, S=90, seed=29, h=200000, max_points=0, allow=False, edit=_member3_invalid)
    # f. many members
    s["f_ebe_4096_64"] = dict(variant="ebe", C=2, E=4096, S=64, seed=61, h=200000, max_points=0, allow=False)
    s["f_ebe_4096_65"] = dict(variant="ebe", C=2, E=4096, S=65, seed=62, h=200000, max_points=0, allow=False)
    s["f_ebesc_4097"] = dict(variant="ebesc", C=2, E=4097, S=5, seed=63, h=200000, max_points=0, allow=False)
    s["f_ebe_4097"] = dict(variant="ebe", C=2, E=4097, S=5, seed=64, h=200000, max_points=0, allow=False)
    s["f_utem_260"] = dict(variant="utem", C=2, E=260, S=130, seed=65, h=200000, max_points=0, allow=False)
    # i. spread at the floor
    for v in ("ebe", "utem"):
        s["i_" + v] = dict(variant=v, C=60, E=6, S=40, seed=43, h=40000, max_points=0, allow=False, edit=_spread_at_the_floor)
    # k. singular systems: 6 observations (k_ensi_multi) and 70 (k_ensi_multi_huge)
    s["k_sing_lds"] = dict(variant="ebesc", C=4, E=5, S=6, seed=71, h=200000, max_points=0, allow=False, edit=_two_obs_coincide)
    s["k_sing_huge"] = dict(variant="ebesc", C=4, E=5, S=70, seed=72, h=200000, max_points=0, allow=False, edit=_two_obs_coincide)
    return s


SPECS = _specs()


@functools.lru_cache(maxsize=None)
def case(name):
    """the named case; shared between the tests and never written to"""
    c = make_case(**SPECS[name])
    for val in c.values():
        val.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """the expected values of a named case, computed once: the oracle's, or the committed LAPACK restatement where the oracle's
    eigen-solver needs more than ten seconds (f_utem_260: tools/make_ensi_multi_edge_fixtures.py)"""
    c = case(name)
    if name == "f_utem_260":
        z = np.load(UTEM260_FIXTURE)
        for key in ("background", "pobs", "plat"):      # the fixture belongs to exactly these inputs
            np.testing.assert_array_equal(z[key], c[key])
        ref = z["expected"]
    else:
        ref = oracle(c)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference_allowing_extrapolation(name):
    ref = oracle(with_params(case(name), allow=True))
    ref.setflags(write=False)
    return ref


def changed_fraction(a, b):
    """share of the values that differ between two results (NaN against NaN counts as equal)"""
    return float(np.mean(~((a == b) | (np.isnan(a) & np.isnan(b)))))


@functools.lru_cache(maxsize=None)
def assert_not_vacuous(name):
    """What keeps a named case from being vacuous, asserted on the inputs and the reference alone (never on the code under test):
    the path it is meant to reach is reached, and the edge it is meant to show is visible in the expected values."""
    c, ref = case(name), reference(name)
    bg, letter, variant = c["background"], name[0], str(c["variant"])
    mp = int(c["params"][3])
    rows = (ref != bg).any(axis=1)
    if letter == "a":      # the clamp changes at least 5 % of the values
        assert changed_fraction(ref, reference_allowing_extrapolation(name)) >= 0.05
    elif letter == "b":    # at least 20 grid points on each side of the 64 selected observations, no rho tie
        counts, tie = selection_counts(c)
        assert (counts <= 64).sum() >= 20 and (counts > 64).sum() >= 20 and counts.min() > 0 and not tie
    elif letter == "c":    # every grid point selects exactly max_points
        counts, tie = selection_counts(c)
        assert (counts == mp).all() and not tie
    elif letter == "d":    # every observation is used at every grid point; the members are all valid, or all but member 3
        counts, _ = selection_counts(c)
        assert (counts == c["plat"].size).all()
        bad = [e for e in range(bg.shape[1]) if not np.isfinite(c["pbackground_corr"][:, e]).all()]
        assert bad == ([3] if name == "d_66gap" else [])
    elif letter == "e":    # more candidates than EBIG_CAND = 8192 at every grid point
        counts, tie = selection_counts(with_params(c, max_points=0))
        assert (counts > 8192).all() and not tie
    elif letter == "f":    # every observation in range
        counts, _ = selection_counts(c)
        assert (counts == c["plat"].size).all()
    elif letter == "g":    # more grid points than the 2048 workgroups, and work at (nearly) all of them
        assert bg.shape[0] > 2048 and rows[2048:].mean() > 0.9
    elif letter == "h":    # finite everywhere; one member: ebe and utem return the background, ebesc changes every grid point
        assert np.isfinite(ref).all()
        if bg.shape[1] == 1:
            assert rows.all() if variant == "ebesc" else not rows.any()
        else:
            assert rows.mean() > 0.9
    elif letter == "i":    # no NaN, and more than half the values change
        assert not np.isnan(ref).any() and changed_fraction(ref, bg) > 0.5
    elif letter == "j":
        assert not np.isnan(ref).any()
        if name.startswith("j_far"):
            far = np.zeros(rows.size, bool)
            far[FAR_CELLS] = True
            assert rows[~far].all() and not rows[far].any()
        else:
            assert rows.all()
        if name.startswith("j_nan"):   # every dropped observation is in range of a grid point: with a number in its place the answer differs
            d = dict(c)
            d["pobs"] = np.where(np.isnan(c["pobs"]), F(0.5), c["pobs"])
            assert changed_fraction(oracle(d), ref) > 0.5
    else:
        raise KeyError(name)
    assert rows.any() or (letter == "h" and bg.shape[1] == 1)
    return True
