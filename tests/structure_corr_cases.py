"""The cases of tests/test_gpu_structure_corr_many.py: structures, first points and the pool of second points.

A case names a structure function and the first point(s) it is asked at.  Every case shares one recipe for its 1000 second points,
laid out around the first point on a 0.01 degree lattice (about 1.1 km in latitude, 0.56 km in longitude at 60 N) for scales of
h = 10 km; the list of n points, the Points of n and the Y x X Grid of a test are the first n (Y * X) points of that pool, so one
set of pairwise scalar values serves them all.  The pool is mixed so that no case passes vacuously, whatever the kernel:

  35 %  at the first point's own position with another elevation (eighths of a metre) and land-area fraction (eighths): the only
        second points a LinearStructure correlates with (its localization distance is 0, structure.cpp:902-904), values in (0, 1)
        through the vertical and the laf factor
  40 %  within 6 lattice steps (under 7.5 km: inside the Cressman radius and every localization distance): values in (0, 1)
  20 %  within 45 steps (50 km): on both sides of the Barnes localization distance (36 km, 15 km with hmax)
   5 %  450 to 600 steps north or south (500 to 670 km): beyond every localization distance (Powerlaw: 392 km), exactly 0
  10 % of the elevations and 10 % of the land-area fractions are NaN (structure.cpp:206-213); point 0 IS the first point.

`build(g)` makes the structure with the python mirror `g`; `oracle(O, lat, lon)` the scalar oracle structure it amounts to at a
first point (tests/test_structure_corr_cases_oracle.py checks the conditions above with it, without a GPU).
"""
import ctypes as C

import numpy as np

H, V, W = 10000.0, 200.0, 0.5
N = 1000
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)          # the wave and block edges of a 256-lane grid-stride kernel
GRIDS = ((1, 1), (5, 7), (17, 19))
P1_ELEV, P1_LAF = 100.0, 0.5
CENTRE = (60.0, 10.0)
# the 6 x 5 grid of a spatially varying structure, h varying by +-30 % from cell to cell, and three first points in three of its cells
FIELD_LATS, FIELD_LONS = np.linspace(59.55, 60.55, 6), np.linspace(9.0, 11.0, 5)
FIELD_H = (H * (1 + 0.3 * np.cos(np.arange(30) * 2.4))).reshape(6, 5).astype(np.float32)
FIELD_V = (V * (1 + 0.3 * np.sin(np.arange(30) * 1.7))).reshape(6, 5).astype(np.float32)
FIELD_W = np.full((6, 5), W, np.float32)
SPATIAL_CENTRES = ((60.0, 10.0), (60.22, 10.47), (59.68, 9.03))


def pool(centre, seed=2024):
    """lats, lons, elevs, lafs (float64 arrays of N) around centre = (lat, lon)"""
    rng = np.random.default_rng(seed)
    where = rng.choice(4, N, p=[0.35, 0.40, 0.20, 0.05])
    where[0] = 0
    di, dj = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for k, reach in ((1, 6), (2, 45)):
        m = where == k
        di[m], dj[m] = rng.integers(-reach, reach + 1, m.sum()), rng.integers(-reach, reach + 1, m.sum())
    di[(where == 1) & (di == 0) & (dj == 0)] = 1
    far = where == 3
    di[far], dj[far] = rng.choice([-1, 1], far.sum()) * rng.integers(450, 601, far.sum()), rng.integers(-45, 46, far.sum())
    lats = (np.round(centre[0] * 100) + di) / 100
    lons = (np.round(centre[1] * 100) + dj) / 100
    here = where == 0
    elevs = np.where(here, P1_ELEV + rng.integers(1, 8, N) / 8, P1_ELEV + rng.integers(-300, 301, N)).astype(np.float64)
    lafs = np.where(here, rng.choice([0, 0.125, 0.25, 0.375, 0.625, 0.75, 0.875, 1.0], N), rng.integers(0, 9, N) / 8)
    elevs[rng.random(N) < 0.1] = np.nan
    lafs[rng.random(N) < 0.1] = np.nan
    lats[0], lons[0], elevs[0], lafs[0] = centre[0], centre[1], P1_ELEV, P1_LAF
    return lats, lons, elevs, lafs


# the first point with everything, without an elevation, without a land-area fraction
P1_VARIANTS = {"full": (P1_ELEV, P1_LAF), "nan_elev": (np.nan, P1_LAF), "nan_laf": (P1_ELEV, np.nan)}
# (variant of the first point, background): both flags with the full point, each NaN variant under one of them
COMBOS = (("full", 0), ("full", 1), ("nan_elev", 0), ("nan_laf", 1))


def _field_grid(g):
    lats, lons = np.meshgrid(FIELD_LATS, FIELD_LONS, indexing="ij")
    return g.Grid(lats, lons)


def _field_index(O, lat, lon):
    """nearest cell of the field grid by chord distance, as Grid.get_nearest_neighbour finds it"""
    lats, lons = np.meshgrid(FIELD_LATS, FIELD_LONS, indexing="ij")
    x, y, z = O.convert_coordinates(lats.ravel(), lons.ravel(), 0)
    qx, qy, qz = O.convert_coordinates([lat], [lon], 0)
    d = (x.astype(np.float64) - qx[0]) ** 2 + (y.astype(np.float64) - qy[0]) ** 2 + (z.astype(np.float64) - qz[0]) ** 2
    return np.unravel_index(int(np.argmin(d)), (6, 5))


class Case:
    def __init__(self, name, build, oracle, centres=(CENTRE,), cv=False):
        self.name, self.build, self.oracle, self.centres, self.cv = name, build, oracle, centres, cv

    def __repr__(self):
        return self.name


def _scalar(kind, h=H, v=V, w=W, hmax=np.nan):
    ctor = kind + "Structure"
    if np.isnan(hmax):
        return Case(kind.lower(), lambda g: getattr(g, ctor)(h, v, w), lambda O, lat, lon: O.Struct(kind, h, v, w))
    return Case(kind.lower() + "_hmax", lambda g: getattr(g, ctor)(h, v, w, hmax), lambda O, lat, lon: O.Struct(kind, h, v, w, hmax))


def _spatial_oracle(O, lat, lon):
    i = _field_index(O, lat, lon)
    s = O.Struct("Barnes", float(FIELD_H[i]), float(FIELD_V[i]), W)
    s.min_rho = 0.0013
    s.loc = float(O.lib().orc_structure_localization_distance(C.c_int(0), C.c_float(FIELD_H[i]), C.c_float(0.0013)))
    return s


def _multiple_field_oracle(O, lat, lon):
    i = _field_index(O, lat, lon)
    return O.Struct.multiple(O.Struct("Barnes", H), O.Struct("Soar", 1.0, float(FIELD_V[i])), O.Struct("Barnes", 1.0, 0.0, W))


CASES = [
    _scalar("Barnes"), _scalar("Cressman"), _scalar("Soar"), _scalar("Toar"), _scalar("Powerlaw"),
    _scalar("Linear", 0.5, 0.5, 0.5),                    # (a LinearStructure's scales are minimum correlations)
    _scalar("Barnes", hmax=15000.0),
    Case("multiple", lambda g: g.MultipleStructure(g.SoarStructure(H), g.ToarStructure(1.0, V), g.PowerlawStructure(1.0, 0.0, W)),
         lambda O, lat, lon: O.Struct.multiple(O.Struct("Soar", H), O.Struct("Toar", 1.0, V), O.Struct("Powerlaw", 1.0, 0.0, W))),
    Case("cross_validation", lambda g: g.CrossValidation(g.BarnesStructure(H, V, W), 2000.0),
         lambda O, lat, lon: O.Struct("Barnes", H, V, W).cross_validation(2000.0), cv=True),
    Case("spatial_barnes", lambda g: g.BarnesStructure(_field_grid(g), FIELD_H, FIELD_V, FIELD_W), _spatial_oracle, SPATIAL_CENTRES),
    Case("multiple_field_v",
         lambda g: g.MultipleStructure(g.BarnesStructure(H), g.SoarStructure(_field_grid(g), np.ones((6, 5)), FIELD_V, FIELD_W),
                                       g.BarnesStructure(1.0, 0.0, W)),
         _multiple_field_oracle, SPATIAL_CENTRES[:2]),
]


def vacuous(values, has_p1, cv_background):
    """why these expected values would let a broken kernel pass (None if they would not): fewer than a quarter strictly inside
    (0, 1), no exact 0, or -- with the first point in the set -- no exact 1 at it.  A CrossValidation's corr_background is 0 at the
    first point itself by definition (structure.cpp:918-925): there the 1 cannot exist and the value at the first point must be 0."""
    v = np.asarray(values, np.float32)
    inside = np.count_nonzero((v > 0) & (v < 1))
    if 4 * inside < v.size:
        return "only %d of %d values inside (0, 1)" % (inside, v.size)
    if not np.any(v == 0):
        return "no value is exactly 0"
    if has_p1 and v[0] != (0 if cv_background else 1):
        return "the value at the first point itself is %r" % float(v[0])
    return None
