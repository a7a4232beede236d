"""Case builders of the radius-query edge suites (tests/test_gpu_radius_edges.py on the GPU, tests/test_radius_cases_oracle.py on the
CPU): deterministic point sets for count, gridding, gridding_nearest, get_neighbours*, get_closest_neighbours, distance and nearest at
the membership boundaries, axis pairs, segment lengths, degenerate index geometries and path thresholds of gridpp_amd/csrc/radius.hip,
radius_csr.h and the nearest kernels of runtime.hip; their references from the C oracle (linear scans that know nothing of bins, rings
or wavefronts); a numpy restatement of the host index build (gpp_build_obs_index) that shows which bins and row segments a query of a
case walks; and restatements of the membership test with one comparison changed.  Nothing here imports the GPU package."""
import functools

import numpy as np

F = np.float32
NAN, INF = F(np.nan), F(np.inf)
GEODETIC, CARTESIAN = 0, 1
STATS = ("Mean", "Sum", "Count", "Min", "Max", "Median", "Std", "Variance")
STREAMING = tuple(s for s in STATS if s != "Median")          # one-pass kernels; Median always takes the CSR path
BITWISE = ("Mean", "Sum", "Count", "Min", "Max", "Median")      # with quarter_values: every partial sum is exact in any order
SPREAD_TOL = dict(rtol=1e-5, atol=1e-5)                         # Std / Variance: tests/test_gpu_radius_parity.py
ARC_TOL = dict(rtol=1e-5, atol=0.05)                            # great-circle distances: tests/test_gpu_radius_parity.py


def _o():
    from oracle import oracle as O
    return O


def stat_id(name):
    from tests import refapi
    return getattr(refapi, name)


def quarter_values(n, seed, nan_every=0):
    """multiples of 0.25 in [-64, 64]: float32 sums of up to 2^16 of them are exact whatever the order"""
    v = (np.random.default_rng(seed).integers(-256, 257, n) * 0.25).astype(F)
    if nan_every:
        v[nan_every // 2::nan_every] = NAN
    return v


def narrow(values):
    """The values Std and Variance are run on: the same multiples of 0.25 brought into [-4, 4] (NaN and inf stay).  The kernels and the oracle
    use the reference's shifted sums (util.cpp:50-76: d = v - K with K the first valid value met, var = sum(d^2) / n - (sum(d) / n)^2) and meet
    the neighbours in different orders, so their K differ.  With |d| <= 8 a multiple of 0.25, every partial sum of d and of d^2 (multiples of
    1/16, at most 64 n) is exact in float32 for lists of up to 2^14 values; what is left are the roundings of the two divisions, the square and
    the difference: |error| <= 4 u (sum(d^2) / n + mean_d^2) = 4 u (var + 2 mean_d^2) with u = 2^-24.  A list of one repeated value has d = 0
    throughout (exact); the random lists lie around 0 with var about 5, so |mean_d| <= 4 + |mean| and the bound stays below
    4 u (var + 50) < 1e-5 + 1e-5 var, the tolerance of tests/test_gpu_radius_parity.py.  Values spread over [-64, 64] do not allow this: their
    sums of d^2 round at every step, and lists of 400 points were measured 1.2e-5 apart (relative) between the two orders."""
    v = np.asarray(values, F)
    out = v.copy()
    ok = np.isfinite(v)
    out[ok] = np.round(v[ok] * 0.25) * 0.25
    return out


class Case:
    """input set (ilat, ilon), output locations (olat, olon; oshape for a Grid), values, the (radius, min_num) rows to run"""

    def __init__(self, name, ctype, ilat, ilon, olat, olon, values, rows, oshape=None, ishape=None):
        self.name, self.ctype = name, ctype
        self.ilat, self.ilon = np.asarray(ilat, F).ravel(), np.asarray(ilon, F).ravel()
        self.olat, self.olon = np.asarray(olat, F).ravel(), np.asarray(olon, F).ravel()
        self.values = np.asarray(values, F)
        self.spread_values = narrow(self.values)
        self.rows = tuple((float(F(r)), int(m)) for r, m in rows)
        self.oshape, self.ishape = oshape, ishape
        assert self.values.size == self.ilat.size

    @functools.cached_property
    def ipts(self):
        return _o().Pts(self.ilat, self.ilon, ctype=self.ctype)

    @functools.cached_property
    def opts(self):
        return _o().Pts(self.olat, self.olon, ctype=self.ctype)

    @functools.lru_cache(maxsize=None)
    def count(self, radius, reverse=False):
        a, b = (self.opts, self.ipts) if reverse else (self.ipts, self.opts)
        out = _o().count(a, b, radius)
        out.setflags(write=False)
        return out

    def values_for(self, stat):
        return self.spread_values if stat in ("Std", "Variance") else self.values

    @functools.lru_cache(maxsize=None)
    def gridding(self, radius, min_num, stat):
        out = _o().gridding(self.opts, self.ipts, self.values_for(stat), radius, min_num, stat_id(stat))
        out.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def neighbours(self, q, radius, include_match):
        out = _o().get_neighbours(self.ipts, float(self.olat[q]), float(self.olon[q]), radius, include_match)
        out.setflags(write=False)
        return out

    def chord(self, q, idx):
        """float32 chord from query q to the input points idx, in the operation order of visit_radius"""
        p, o = self.ipts, self.opts
        dx, dy, dz = p.x[idx] - o.x[q], p.y[idx] - o.y[q], p.z[idx] - o.z[q]
        return np.sqrt(dx * dx + dy * dy + dz * dz)

    @functools.lru_cache(maxsize=None)
    def closest(self, q, num, include_match=True):
        """get_closest_neighbours: float32 squared chord, nearest first, ties -> lower index, exact matches skipped on request"""
        p, o = self.ipts, self.opts
        dx, dy, dz = p.x - o.x[q], p.y - o.y[q], p.z - o.z[q]
        s2 = dx * dx + dy * dy
        s2 = s2 + dz * dz
        order = np.argsort(s2, kind="stable")
        if not include_match:
            same = (p.x == o.x[q]) & (p.y == o.y[q]) & (p.z == o.z[q])
            order = order[~same[order]]
        return order[:max(num, 0)].astype(np.int32)

    @functools.lru_cache(maxsize=None)
    def distance(self, num, query_first):
        out = _o().distance(self.ipts, self.opts, num, query_first)
        out.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def nearest(self):
        out = _o().nearest(self.ipts, self.opts, self.values)
        out.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def gridding_nearest(self, min_num, stat):
        out = _o().gridding_nearest(self.opts, self.ipts, self.values, min_num, stat_id(stat))
        out.setflags(write=False)
        return out

    @functools.cached_property
    def index(self):
        return Index(self.ipts)


# ---- the host index build, restated (gpp_build_obs_index in gridpp_amd/csrc/oi.hip; the device build uses the same formulas) ------
class Index:
    def __init__(self, pts):
        ax = (pts.x, pts.y, pts.z)
        S = pts.n
        lo = [F(a.min()) for a in ax]
        hi = [F(a.max()) for a in ax]
        ext = [F(h - l) for h, l in zip(hi, lo)]
        order = sorted(range(3), key=lambda d: -ext[d])                     # (stable, like the insertion sort std::sort does on 3)
        a, b = min(order[0], order[1]), max(order[0], order[1])
        ea, eb = max(float(hi[a]) - float(lo[a]), 1e-3), max(float(hi[b]) - float(lo[b]), 1e-3)
        s = max(np.sqrt(4.0 * ea * eb / max(S, 1)), max(ea, eb) / 2048.0)
        self.axes = (a, b)
        self.tied_axes = ext[order[1]] == ext[order[2]]                     # then the second axis is the sort's choice
        self.nbx, self.nby = max(1, min(2048, int(np.ceil(ea / s)))), max(1, min(2048, int(np.ceil(eb / s))))
        self.amin, self.bmin, self.inv_s, self.s = lo[a], lo[b], F(1.0 / s), s
        self.amax, self.bmax = hi[a], hi[b]
        self.S = S
        bx, by = self.bin_a(ax[a]), self.bin_b(ax[b])
        self.bin = by * self.nbx + bx
        self.start = np.concatenate(([0], np.cumsum(np.bincount(self.bin, minlength=self.nbx * self.nby))))
        self.order = np.argsort(self.bin, kind="stable")                     # index order inside a bin

    def _bin(self, v, lo, nb):
        f = np.floor((np.asarray(v, F) - lo) * self.inv_s)                   # float32 throughout, as bin_of
        return np.clip(f, 0, nb - 1).astype(np.int64)

    def bin_a(self, v):
        return self._bin(v, self.amin, self.nbx)

    def bin_b(self, v):
        return self._bin(v, self.bmin, self.nby)

    def box(self, q3, radius):
        """(bx0, bx1, by0, by1) of visit_radius for a query (x, y, z)"""
        r = F(radius)
        qa, qb = F(q3[self.axes[0]]), F(q3[self.axes[1]])
        return (int(self.bin_a(qa - r)), int(self.bin_a(qa + r)), int(self.bin_b(qb - r)), int(self.bin_b(qb + r)))

    def segments(self, q3, radius):
        """je - js of every bin row the walk visits"""
        bx0, bx1, by0, by1 = self.box(q3, radius)
        return [int(self.start[row * self.nbx + bx1 + 1] - self.start[row * self.nbx + bx0]) for row in range(by0, by1 + 1)]

    def segment_members(self, q3, radius):
        """original indices of every visited segment, in walk order"""
        bx0, bx1, by0, by1 = self.box(q3, radius)
        return [self.order[self.start[row * self.nbx + bx0]:self.start[row * self.nbx + bx1 + 1]] for row in range(by0, by1 + 1)]


def query3(case, q):
    o = case.opts
    return (o.x[q], o.y[q], o.z[q])


# ---- the membership test, restated with one comparison changed -------------------------------------------------------------------
def members(case, q, radius, include_match=True, closed_box=False, open_disc=False):
    """kdtree.cpp:46,53 + :247-260 in float32: strictly inside the box +-radius, chord <= radius (and > 0 without the match)"""
    p, o = case.ipts, case.opts
    r = F(radius)
    if not r > 0 and not closed_box:
        return np.zeros(0, np.int64)
    keep = np.ones(p.n, bool)
    for pc, qc in ((p.x, o.x[q]), (p.y, o.y[q]), (p.z, o.z[q])):
        lo, hi = F(qc - r), F(qc + r)
        keep &= ((pc >= lo) & (pc <= hi)) if closed_box else ((pc > lo) & (pc < hi))
    d = case.chord(q, np.arange(p.n))
    keep &= (d < r) if open_disc else (d <= r)
    if not include_match:
        keep &= d > 0
    return np.nonzero(keep)[0]


# ---- 1. the boundary lattice ------------------------------------------------------------------------------------------------------
LATTICE_N = 21
LATTICE_OFFSETS = (0.0, 1e5, float(2 ** 22))
R5 = F(5)
LATTICE_RADII = (0.0, 1.0, float(np.nextafter(R5, F(0))), 5.0, float(np.nextafter(R5, F(10))), 10.0, 13.0)
LATTICE_CENTRE = (LATTICE_N // 2) * LATTICE_N + LATTICE_N // 2              # the centre node, as an output location of "nodes"
LATTICE_QUERIES = (0, LATTICE_N - 1, LATTICE_CENTRE, LATTICE_CENTRE + 3, LATTICE_N * LATTICE_N - 1)


@functools.lru_cache(maxsize=None)
def lattice_case(offset, queries):
    """Cartesian, 21 x 21 nodes 1 m apart; queries = "nodes" (the lattice itself) or "centres" (the 20 x 20 cell centres)"""
    k = np.arange(LATTICE_N, dtype=np.float64) + offset
    ilat, ilon = np.meshgrid(k, k, indexing="ij")
    assert np.array_equal(ilat.astype(F).astype(np.float64), ilat)          # every coordinate is exact in float32
    if queries == "nodes":
        olat, olon = ilat, ilon
    else:
        olat, olon = np.meshgrid(k[:-1] + 0.5, k[:-1] + 0.5, indexing="ij")
        assert np.array_equal(olat.astype(F).astype(np.float64), olat)
    rows = [(r, m) for r in LATTICE_RADII for m in (0, 5)]
    return Case("lattice-%g-%s" % (offset, queries), CARTESIAN, ilat, ilon, olat, olon, quarter_values(ilat.size, 5, 17), rows,
                oshape=olat.shape, ishape=ilat.shape)


# ---- 2. axis pairs ---------------------------------------------------------------------------------------------------------------
AXIS_CASES = {"cartesian": (0, 1), "geo_60N_10E": (0, 1), "geo_equator_0E": (1, 2), "geo_equator_90E": (0, 2), "geo_dateline": None,
              "geo_polar_cap": None}


@functools.lru_cache(maxsize=None)
def axis_case(name):
    rng = np.random.default_rng(sorted(AXIS_CASES).index(name) + 40)
    n, nq = (3000, 300) if AXIS_CASES[name] else (2000, 300)
    u, v, qu, qv = rng.random(n), rng.random(n), rng.random(nq) * 1.2 - 0.1, rng.random(nq) * 1.2 - 0.1     # some outside the hull
    ctype, radii = GEODETIC, (800.0, 7000.0, 3e5)
    if name == "cartesian":
        ctype = CARTESIAN
        ilat, ilon, olat, olon = 1e5 * u, 1e5 * v, 1e5 * qu, 1e5 * qv
    elif name == "geo_dateline":
        ilat, olat = 59 + u, 59 + qu
        ilon, olon = 179 + 2 * v, 179 + 2 * qv
        ilon, olon = np.where(ilon > 180, ilon - 360, ilon), np.where(olon > 180, olon - 360, olon)
    elif name == "geo_polar_cap":
        ilat, olat = 89 + u, np.minimum(88.9 + 1.1 * rng.random(nq), 90)
        ilon, olon = 360 * v - 180, 360 * rng.random(nq) - 180
        radii = (800.0, 7000.0, 3e5)
    else:
        lat0, lon0 = {"geo_60N_10E": (59.5, 9.0), "geo_equator_0E": (-0.5, -1.0), "geo_equator_90E": (-0.5, 89.0)}[name]
        ilat, ilon, olat, olon = lat0 + u, lon0 + 2 * v, lat0 + qu, lon0 + 2 * qv
    ilat, ilon, olat, olon = (np.array(a, F) for a in (ilat, ilon, olat, olon))
    olat[:20], olon[:20] = ilat[:20], ilon[:20]                              # exact matches
    return Case(name, ctype, ilat, ilon, olat, olon, quarter_values(n, 6, 41), [(radii[0], 0), (radii[1], 3), (radii[2], 7)])


# ---- 3. chunk lengths of k_radius_statistic_wave ----------------------------------------------------------------------------------
CHUNK_LENGTHS = (1, 63, 64, 65, 127, 128, 129)
CHUNK_RADII = (1.0, 200.0)


@functools.lru_cache(maxsize=None)
def chunk_case():
    """Cartesian.  Site k holds CHUNK_LENGTHS[k] points of one bin: the first 64 (or all, if fewer) coincide with the site and are hit at radius 1
    (a full chunk), of the others every fifth one is (sparse chunks); the rest sit 3 m beside it, in the same bin.  The sites are bin centres of
    consecutive bin rows (the index has 13 x 13 bins), two anchors fix the extents.  Query k is site k: at radius 1 it walks one row, whose segment is exactly the cluster.
    Lane 0 and lane 63 of the first chunk and lane 0 of the second hold a NaN value."""
    S = sum(CHUNK_LENGTHS) + 2
    E = 1000.0
    s = np.sqrt(4.0 * E * E / S)
    lat, lon, val, sites = [0.0, E], [0.0, E], [1.0, 2.0], []
    v = quarter_values(S, 7)
    for k, L in enumerate(CHUNK_LENGTHS):
        sx, sy = (k + 1.5) * s, (10.5 - k) * s                        # Cartesian: y = first coordinate (axis b), x = second (axis a)
        sites.append((sx, sy))
        for i in range(L):
            hit = i < 64 or (i - 64) % 5 == 0
            lat.append(sx + (0.0 if hit else 3.0))
            lon.append(sy)
            val.append(NAN if i in (0, 63, 64) else v[len(val)])
    olat, olon = [a for a, _ in sites], [b for _, b in sites]
    return Case("chunks", CARTESIAN, lat, lon, olat, olon, val, [(r, m) for r in CHUNK_RADII for m in (0, 64)])


# ---- 4. degenerate and clamped geometry -------------------------------------------------------------------------------------------
DEGENERATE = ("one", "two", "three", "four", "five", "coincident500", "line_lat1000", "line_lon1000", "geo_one", "geo_five")


@functools.lru_cache(maxsize=None)
def degenerate_case(name):
    """Queries: the corners and the middles of the sides of its bounding box, the set's centre, its first and last point, the points with the
    smallest and the largest x, y and z (on amin / amax of the binned axes), and eight queries ten extents outside each side and corner.  Radii: half an extent (reaches nothing from outside), 10.5 extents (reaches in),
    a radius that covers everything."""
    geo = name.startswith("geo_")
    base = {"one": 1, "two": 2, "three": 3, "four": 4, "five": 5, "geo_one": 1, "geo_five": 5}.get(name)
    rng = np.random.default_rng(DEGENERATE.index(name) + 90)
    if base:
        lat, lon = np.round(rng.random(base) * 400) * 0.25, np.round(rng.random(base) * 400) * 0.25
    elif name == "coincident500":
        lat, lon = np.full(500, 250.0), np.full(500, 125.0)
    elif name == "line_lat1000":
        lat, lon = np.full(1000, 40.0), np.arange(1000) * 0.5
    else:
        lat, lon = np.arange(1000) * 0.5, np.full(1000, 40.0)
    if geo:
        lat, lon = 60 + lat * 1e-3, 10 + lon * 2e-3                          # a box of 0.1 x 0.2 degrees
    ext = max(lat.max() - lat.min(), lon.max() - lon.min()) or (1e-3 if geo else 1.0)
    la0, la1, lo0, lo1 = lat.min(), lat.max(), lon.min(), lon.max()
    lam, lom = 0.5 * (la0 + la1), 0.5 * (lo0 + lo1)
    near = [(la0, lom), (la1, lom), (lam, lo0), (lam, lo1), (lam, lom), (la0, lo0), (la1, lo1), (lat[0], lon[0]), (lat[-1], lon[-1])]
    xyz = _o().convert_coordinates(lat, lon, GEODETIC if geo else CARTESIAN)
    near += [(lat[k], lon[k]) for a in xyz for k in (int(np.argmin(a)), int(np.argmax(a)))]      # on amin / amax of whichever axes are binned
    far = [(lam + 10 * ext * dy, lom + 10 * ext * dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]
    olat, olon = zip(*(near + far))
    metres = ext * (111e3 if geo else 1.0)
    rows = [(0.5 * metres, 0), (10.5 * metres * (2.2 if geo else 1.0), 1), (40 * metres, 2)]
    n = lat.size
    return Case(name, GEODETIC if geo else CARTESIAN, lat, lon, olat, olon, quarter_values(n, 8, 7 if n > 10 else 0), rows)


DEGENERATE_FAR = range(15, 23)            # the eight outside queries of a degenerate case


# ---- 5. min_num and the statistics of special lists ---------------------------------------------------------------------------------
LIST_KINDS = ("all_nan", "all_pinf", "all_ninf", "mixed_inf", "one_valid", "all_equal", "ordinary", "empty")
LIST_C = 6                                # neighbours of every location but the empty one
LIST_RADIUS = 10.0
LIST_MIN_NUMS = (0, LIST_C - 1, LIST_C, LIST_C + 1)


@functools.lru_cache(maxsize=None)
def lists_case():
    """Cartesian: location k at (1000 k, 0) with LIST_C points within 10 m of it (none for "empty"), values by kind"""
    lat, lon, val = [], [], []
    fill = {"all_nan": [NAN] * 6, "all_pinf": [INF] * 6, "all_ninf": [-INF] * 6, "mixed_inf": [INF, -INF, NAN, INF, -INF, NAN],
            "one_valid": [NAN, NAN, NAN, 7.25, NAN, NAN], "all_equal": [-3.5] * 6, "ordinary": [1.0, -2.25, 8.5, 8.5, NAN, 0.0], "empty": []}
    for k, kind in enumerate(LIST_KINDS):
        for i, v in enumerate(fill[kind]):
            lat.append(1000.0 * k + (i - 2.5))
            lon.append(float(i % 3))
            val.append(v)
    olat, olon = 1000.0 * np.arange(len(LIST_KINDS)), np.zeros(len(LIST_KINDS))
    return Case("lists", CARTESIAN, lat, lon, olat, olon, val, [(LIST_RADIUS, m) for m in LIST_MIN_NUMS])


# ---- 6. the device-built index ----------------------------------------------------------------------------------------------------
BIG_N = (1 << 17) + 3


@functools.lru_cache(maxsize=None)
def big_case():
    rng = np.random.default_rng(17)
    ilat, ilon = np.round(rng.random(BIG_N) * 4e5) * 0.25, np.round(rng.random(BIG_N) * 4e5) * 0.25        # a 100 km square, quarter metres
    olat, olon = np.round((rng.random(360) * 1.1 - 0.05) * 4e5) * 0.25, np.round((rng.random(360) * 1.1 - 0.05) * 4e5) * 0.25
    olat[:20], olon[:20] = ilat[:20], ilon[:20]
    return Case("big", CARTESIAN, ilat, ilon, olat, olon, quarter_values(BIG_N, 9, 53), [(300.0, 0), (1500.0, 80), (0.25, 1)])


# ---- 7. gridding_nearest ----------------------------------------------------------------------------------------------------------
NEAREST_SIZES = (1, 2, 64, 1024, 1025, 2070)


def _lattice_of(no):
    w = int(np.ceil(np.sqrt(no)))
    k = np.arange(no)
    return (k // w).astype(np.float64), (k % w).astype(np.float64), w


@functools.lru_cache(maxsize=None)
def nearest_case(no, kind="ties"):
    """Cartesian; the output locations are the first `no` nodes of a unit lattice w wide.  "ties": 700 input points at multiples of half a cell in
    and around it -- nodes, edge middles (two nodes equally near) and cell centres (four).  "one": every input point nearest to location no // 2."""
    olat, olon, w = _lattice_of(no)
    rng = np.random.default_rng(no)
    h = (no + w - 1) // w
    if kind == "ties":
        ilat, ilon = rng.integers(-2, 2 * h + 1, 700) * 0.5, rng.integers(-2, 2 * w + 1, 700) * 0.5
    else:
        ilat, ilon = olat[no // 2] + rng.integers(-3, 4, 90) * 0.125, olon[no // 2] + rng.integers(-3, 4, 90) * 0.125
    return Case("nearest-%d-%s" % (no, kind), CARTESIAN, ilat, ilon, olat, olon, quarter_values(ilat.size, no, 13), [])


def tie_candidates(case, i):
    """the output locations at the smallest float32 squared chord from input point i (more than one: a tie)"""
    p, o = case.ipts, case.opts
    dx, dy, dz = o.x - p.x[i], o.y - p.y[i], o.z - p.z[i]
    s2 = dx * dx + dy * dy
    s2 = s2 + dz * dz
    return np.nonzero(s2 == s2.min())[0]


# ---- 8. k nearest ---------------------------------------------------------------------------------------------------------------------
KNN_N = 40
KNN_NUMS = (0, 1, KNN_N - 1, KNN_N, KNN_N + 1)


@functools.lru_cache(maxsize=None)
def knn_lattice_case():
    """40 nodes of a 5 x 8 unit lattice; queries on nodes, edge middles, cell centres and outside: ties at every rank"""
    ilat, ilon = np.meshgrid(np.arange(5.0), np.arange(8.0), indexing="ij")
    olat, olon = np.meshgrid(np.arange(-1, 5.5, 0.5), np.arange(-1, 8.5, 0.5), indexing="ij")
    return Case("knn-lattice", CARTESIAN, ilat, ilon, olat, olon, quarter_values(KNN_N, 3), [], oshape=olat.shape, ishape=ilat.shape)


@functools.lru_cache(maxsize=None)
def duplicates_case(dup):
    """20 random points plus `dup` exact copies of point 4; query 0 is that point, query 1 lies elsewhere"""
    rng = np.random.default_rng(dup)
    lat, lon = np.round(rng.random(20) * 400) * 0.25, np.round(rng.random(20) * 400) * 0.25
    lat, lon = np.concatenate((lat, np.full(dup, lat[4]))), np.concatenate((lon, np.full(dup, lon[4])))
    return Case("dup-%d" % dup, CARTESIAN, lat, lon, [lat[4], 33.0], [lon[4], 44.0], quarter_values(lat.size, 2), [])


CLUSTER_NUMS = (1, 299, 301, 600)


@functools.lru_cache(maxsize=None)
def clusters_case(per_cluster=300):
    """Cartesian: two clusters of `per_cluster` points in 10 m squares 3000 m apart along the second coordinate -- an index of one bin row whose
    clusters lie more than 200 bins apart; queries at the midpoint, beside each cluster, inside each, and beyond both ends"""
    rng = np.random.default_rng(per_cluster)
    n = per_cluster
    lat = np.round(rng.random(2 * n) * 40) * 0.25
    lon = np.round(rng.random(2 * n) * 40) * 0.25 + np.repeat([0.0, 3000.0], n)
    olat = [5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 2.0]
    olon = [1505.0, 30.0, 2980.0, 5.0, 3005.0, -900.0, 4000.0, 1400.25]
    return Case("clusters-%d" % n, CARTESIAN, lat, lon, olat, olon, quarter_values(2 * n, 4), [])


# ---- 9. the batched entry point ------------------------------------------------------------------------------------------------------
BATCH_RADIUS = 5.0
SENTINEL_I, SENTINEL_F = -77, F(-7.5)


def batch_case():
    """the boundary lattice with its five named queries"""
    c = lattice_case(0.0, "nodes")
    q = np.array(LATTICE_QUERIES)
    lists = [c.neighbours(int(k), BATCH_RADIUS, True) for k in q]
    counts = np.array([len(l) for l in lists], np.int32)
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    idx = np.concatenate(lists).astype(np.int32)
    dist = np.concatenate([c.chord(int(k), l) for k, l in zip(q, lists)]).astype(F)
    return c, q, counts, offsets, idx, dist
