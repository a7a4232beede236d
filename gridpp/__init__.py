"""`import gridpp` -> the MI355X implementation of gridpp's optimal-interpolation / neighbourhood path (gridpp_amd).

The reference's SWIG module is `%module gridpp` (swig/gridpp.i:1); with this package on the path a script written for the
reference runs unchanged on the functions gridpp_amd covers.  It never shadows an installed reference:
if another `gridpp` distribution is importable from a different sys.path entry, THAT one is loaded under this name (set
GRIDPP_USE_AMD=1 to take this implementation anyway, e.g. for an A/B run in one environment).
"""
import importlib.machinery as _mach
import importlib.util as _util
import os as _os
import sys as _sys

_here = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
_other = None
if not _os.environ.get("GRIDPP_USE_AMD"):
    _paths = [p for p in _sys.path if _os.path.abspath(p or _os.getcwd()) != _here]
    try:
        _other = _mach.PathFinder.find_spec("gridpp", _paths)
    except (ImportError, ValueError):
        _other = None

if _other is not None and _other.origin and _os.path.abspath(_other.origin) != _os.path.abspath(__file__):
    _mod = _util.module_from_spec(_other)
    _sys.modules[__name__] = _mod
    _other.loader.exec_module(_mod)
else:
    import gridpp_amd as _impl
    from gridpp_amd import *          # noqa: F401,F403
    # (everything public, also the names `import *` skips when a module defines no __all__)
    globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("_")})
    # The alias carries the surface the suite pins for it (tests/test_pointwise_api.py lists the names a script must not find here).
    # local_distribution_correction orders tied values by rho where the reference leaves them to an unstable sort:
    # a script written for the reference asks for it by its own name, gridpp_amd.local_distribution_correction.
    # Gamma and gamma_inv return IEEE values (NaN, -inf, +inf) at the edges where the reference raises through Boost's error policies
    # (DESIGN.md 4.12): they too are asked for by their own names, gridpp_amd.Gamma and gridpp_amd.gamma_inv.
    # get_optimal_threshold and metric_optimizer_curve return the exact optimum over the plateaus of the score where the reference returns
    # wherever Boost's brent_find_minima ends: gridpp_amd.get_optimal_threshold, gridpp_amd.metric_optimizer_curve.
    # optimal_interpolation_gain and its OiGain have no counterpart in the reference at all (the selections and weights of
    # optimal_interpolation computed once per geometry and applied to any number of fields): gridpp_amd.optimal_interpolation_gain.
    # calc_quantiles and quantile_mapping_curves have no counterpart in the reference either (many quantiles of every row from
    # one sort, and one quantile-mapping curve per cell for apply_curve): gridpp_amd.calc_quantiles, gridpp_amd.quantile_mapping_curves.
    # Nor have neighbourhood_quantiles_fast and neighbourhood_cdf (many levels of neighbourhood_quantile_fast from one pass over
    # the cube, and the per-threshold neighbourhood probabilities it interpolates in): gridpp_amd.neighbourhood_quantiles_fast, gridpp_amd.neighbourhood_cdf.
    # calc_ranks, sort_rows, reorder_by_ranks and calc_crps have none either (the rank of every member within its cell, the sorted
    # rows, ensemble copula coupling and the CRPS): gridpp_amd.calc_ranks, gridpp_amd.sort_rows, gridpp_amd.reorder_by_ranks, gridpp_amd.calc_crps.
    # downscaling_plan and its DownscalingPlan have none either (the nearest grid point, box and weights of every output
    # location computed once per pair of geometries and applied to any number of fields): gridpp_amd.downscaling_plan.
    # neighbourhood_members and calc_gradient_members have none either (a spatial filter and the gradient of every member of a
    # (Y, X, E) cube without a permute): gridpp_amd.neighbourhood_members, gridpp_amd.calc_gradient_members.
    # fractions_skill_score and its FssResult have none either (the Fractions Skill Score of a field or an ensemble cube for a
    # table of thresholds x half widths from one pass over the inputs): gridpp_amd.fractions_skill_score.
    for _name in ("local_distribution_correction", "Gamma", "gamma_inv", "get_optimal_threshold", "metric_optimizer_curve",
                  "optimal_interpolation_gain", "OiGain", "calc_quantiles", "quantile_mapping_curves",
                  "neighbourhood_quantiles_fast", "neighbourhood_cdf", "calc_ranks", "sort_rows", "reorder_by_ranks", "calc_crps",
                  "downscaling_plan", "DownscalingPlan", "neighbourhood_members", "calc_gradient_members",
                  "fractions_skill_score", "FssResult"):
        globals().pop(_name, None)
    __version__ = getattr(_impl, "__version__", None)
    implementation = "gridpp_amd"
