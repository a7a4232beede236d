"""Meshes whose boxes are general quadrilaterals for the weights of gridpp::bilinear, a numpy restatement of which formula
each box takes (gridpp_amd/csrc/bilinear_geom.h: weights / weights_general, src/api/bilinear.cpp:159-313 in the reference),
queries that reach the edges of that solve, and a float64 reference that shares nothing with its quadratic formula.

weights() takes the parallelogram formula whenever both cross products of opposite edges are at most an ABSOLUTE 1e-4, so a
mesh in degrees with millidegree curvature never reaches the general solve however warped it looks: the meshes here have
products of thousands (metres) or of 1e-3 and more (degrees with cells of about 1 degree).

Importing this module needs numpy only; the functions that run the oracle import it when they are called."""
import functools

import numpy as np

F32 = np.float32
F64 = np.float64


# ---- meshes: float64 (lats, lons); callers round to float32 as Grid does ------------------------------------------------------
def _ji(Y, X):
    return np.meshgrid(np.arange(Y, dtype=F64), np.arange(X, dtype=F64), indexing="ij")


def warped_metres(Y, X, seed, x0=0.0, y0=0.0):
    """Cartesian, 2500 m x 1875 m cells rotated by a seeded angle in +-30 degrees, 0.1 % warp per cell.  At a large origin offset
    the float32 coordinates carry half a metre of rounding: the solve must form its differences in float, then go to double."""
    a = np.deg2rad(np.random.default_rng(seed).uniform(-30, 30))
    j, i = _ji(Y, X)
    u = 2500 * (i * np.cos(a) - j * np.sin(a)) + 2.5 * i * j
    v = 1875 * (i * np.sin(a) + j * np.cos(a)) + 1.25 * i * i
    return y0 + v, x0 + u


def warped_degrees(Y, X, seed):
    """Geodetic, cells of about 1 x 0.75 degrees near (20, -10)."""
    a = np.deg2rad(np.random.default_rng(seed).uniform(-30, 30))
    j, i = _ji(Y, X)
    u = i * np.cos(a) - j * np.sin(a) + 4e-3 * i * j
    v = 0.75 * (i * np.sin(a) + j * np.cos(a)) + 2e-3 * i * i
    return 20 + v, -10 + u


def trapezoid(Y, X, axis):
    """Dyadic coordinates (every product of the solve is exact in float) with one pair of edges exactly parallel.  axis 0: rows of
    constant lat that widen with j; axis 1: the same construction with the roles of (lat, j) and (lon, i) exchanged."""
    if axis == 1:
        lons, lats = trapezoid(X, Y, 0)
        return lats.T, lons.T
    j, i = _ji(Y, X)
    return j / 2, (i - (X - 1) / 2) * (0.5 + j / 16)


ORIENTATIONS = ("asis", "flipY", "flipX", "transposed")


def orient(lats, lons, how):
    if how == "asis":
        return lats, lons
    if how == "flipY":
        return lats[::-1], lons[::-1]
    if how == "flipX":
        return lats[:, ::-1], lons[:, ::-1]
    if how == "transposed":
        return lats.T, lons.T
    raise ValueError(how)


# ---- which formula each box takes ---------------------------------------------------------------------------------------------------
def box_corners(lats, lons):
    """float32 corners of every box as get_box names them: 0 = (Y1, X1), 1 = (Y2, X1), 2 = (Y1, X2), 3 = (Y2, X2) -> (xs, ys),
    x = lon, y = lat, each a 4-tuple of (Y - 1, X - 1) arrays"""
    la, lo = np.asarray(lats, F32), np.asarray(lons, F32)
    pick = lambda a: (a[:-1, :-1], a[1:, :-1], a[:-1, 1:], a[1:, 1:])   # noqa: E731
    return pick(lo), pick(la)


def _coefficients(xs, ys):
    """a, b, c, e, f, g of the general solve: float32 differences, then float64"""
    x0, x1, x2, x3 = xs
    y0, y1, y2, y3 = ys
    a, b, c = -x0 + x2, -x0 + x1, x0 - x1 - x2 + x3
    e, f, g = -y0 + y2, -y0 + y1, y0 - y1 - y2 + y3
    assert all(np.asarray(v).dtype == F32 for v in (a, b, c, e, f, g))
    return tuple(np.asarray(v, F64) for v in (a, b, c, e, f, g))


def _is_parallelogram(xs, ys):
    X1, X2, X3, X4 = xs[1], xs[3], xs[0], xs[2]
    Y1, Y2, Y3, Y4 = ys[1], ys[3], ys[0], ys[2]
    vertical = np.abs((X3 - X1) * (Y4 - Y2) - (X4 - X2) * (Y3 - Y1))
    horizontal = np.abs((X2 - X1) * (Y4 - Y3) - (X4 - X3) * (Y2 - Y1))
    assert np.asarray(vertical).dtype == F32 and np.asarray(horizontal).dtype == F32
    return (vertical.astype(F64) <= 1e-4) & (horizontal.astype(F64) <= 1e-4)


def classify(lats, lons):
    """-> counts of boxes per path: parallelogram / both (qa != 0 and qb != 0) / qb0 / qa0, and the largest cross product"""
    xs, ys = box_corners(lats, lons)
    par = _is_parallelogram(xs, ys)
    a, b, c, e, f, g = _coefficients(xs, ys)
    qa, qb = 2 * c * e - 2 * a * g, 2 * c * f - 2 * b * g
    both = ~par & (qa != 0) & (qb != 0)
    qb0 = ~par & ~both & (qb == 0)
    qa0 = ~par & ~both & ~qb0
    return dict(boxes=int(par.size), parallelogram=int(par.sum()), both=int(both.sum()), qb0=int(qb0.sum()), qa0=int(qa0.sum()))


def _in_range(v):
    tol = F32(0.01)
    v = np.asarray(v, F32)
    return (v >= -tol) & (v < F32(1) + tol)


def root_taken(xs, ys, x, y):
    """Does in_range accept the FIRST root of the quadratic?  xs, ys: float32 corners (4-tuples, get_box order) of the box of each
    query, x / y: the float32 query.  -> (alpha_first, beta_first, has_alpha, has_beta): the last two say whether the branch of the
    box solves that unknown by the quadratic at all (qa != 0 / qb != 0); the qa == 0 branch has no second root."""
    a, b, c, e, f, g = _coefficients(xs, ys)
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    d, h = np.asarray(x - xs[0], F64), np.asarray(y - ys[0], F64)
    qa, qb = 2 * c * e - 2 * a * g, 2 * c * f - 2 * b * g
    lin1 = b * e - a * f + d * g - c * h
    lin2 = b * e - a * f - d * g + c * h
    with np.errstate(invalid="ignore", divide="ignore"):
        root = np.sqrt(-4 * (c * e - a * g) * (d * f - b * h) + lin1 * lin1)
        alpha_first = _in_range(-(lin1 + root) / qa)
        beta_first = _in_range((lin2 + root) / qb)
    has_alpha, has_beta = qa != 0, qb != 0
    return alpha_first & has_alpha, beta_first & has_beta, has_alpha, has_beta


# ---- queries ----------------------------------------------------------------------------------------------------------------------------
def queries(lats, lons, n, seed, margin=0.05):
    """-> float32 (qlat, qlon): 200 exact nodes, 200 midpoints of cell edges (the solved weights land a few ulps outside [0, 1]: the
    snap), 4 x 100 points of the first / last cell row and column, the rest uniform over the bounding box plus the margin."""
    rng = np.random.default_rng(seed)
    la, lo = np.asarray(lats, F32).astype(F64), np.asarray(lons, F32).astype(F64)
    Y, X = la.shape
    dlat, dlon = la.max() - la.min(), lo.max() - lo.min()
    qlat = la.min() - margin * dlat + (1 + 2 * margin) * dlat * rng.random(n)
    qlon = lo.min() - margin * dlon + (1 + 2 * margin) * dlon * rng.random(n)
    k = 0

    def put(plat, plon):
        nonlocal k
        m = min(len(plat), n - k)
        qlat[k:k + m], qlon[k:k + m] = plat[:m], plon[:m]
        k += m

    node = np.unique(np.concatenate([[0, X - 1, (Y - 1) * X, Y * X - 1], rng.choice(Y * X, min(200, Y * X), replace=False)]))[:200]
    put(la.ravel()[node], lo.ravel()[node])
    if Y > 1 and X > 1:
        ey, ex = rng.integers(0, Y - 1, 100), rng.integers(0, X, 100)          # edges along Y
        put((la[ey, ex] + la[ey + 1, ex]) / 2, (lo[ey, ex] + lo[ey + 1, ex]) / 2)
        ey, ex = rng.integers(0, Y, 100), rng.integers(0, X - 1, 100)          # edges along X
        put((la[ey, ex] + la[ey, ex + 1]) / 2, (lo[ey, ex] + lo[ey, ex + 1]) / 2)
        for by, bx in ((np.zeros(100, int), rng.integers(0, X - 1, 100)), (np.full(100, Y - 2), rng.integers(0, X - 1, 100)),
                       (rng.integers(0, Y - 1, 100), np.zeros(100, int)), (rng.integers(0, Y - 1, 100), np.full(100, X - 2))):
            u, v = rng.random(100), rng.random(100)
            w = ((1 - u) * (1 - v), u * (1 - v), (1 - u) * v, u * v)
            cs = ((by, bx), (by, bx + 1), (by + 1, bx), (by + 1, bx + 1))
            put(sum(wk * la[c] for wk, c in zip(w, cs)), sum(wk * lo[c] for wk, c in zip(w, cs)))
    return qlat.astype(F32), qlon.astype(F32)


# ---- the float64 reference ------------------------------------------------------------------------------------------------------------
def truth(lats, lons, values, boxes, qlat, qlon, iterations=30):
    """boxes (n, 5) = inside, Y1, X1, Y2, X2 per query.  For every query with a box: invert the bilinear map of the float32 corner
    coordinates in float64 by Newton from (0.5, 0.5), clamp (u, v) to [0, 1], interpolate the float32 corner values in float64.
    -> (value, u, v) with the unclamped (u, v); NaN where the query has no box."""
    la, lo = np.asarray(lats, F32).astype(F64), np.asarray(lons, F32).astype(F64)
    val = np.asarray(values, F32).astype(F64)
    boxes = np.asarray(boxes)
    n = len(boxes)
    out, uu, vv = (np.full(n, np.nan) for _ in range(3))
    m = boxes[:, 0] != 0
    Y1, X1, Y2, X2 = (boxes[m, k] for k in range(1, 5))
    x, y = np.asarray(qlon, F32).astype(F64)[m], np.asarray(qlat, F32).astype(F64)[m]
    c = ((Y1, X1), (Y1, X2), (Y2, X1), (Y2, X2))                     # p(u, v) = c0 (1-u)(1-v) + c1 u (1-v) + c2 (1-u) v + c3 u v
    px, py, pv = ([f[k] for k in c] for f in (lo, la, val))
    ax, bx, cx = px[1] - px[0], px[2] - px[0], px[0] - px[1] - px[2] + px[3]
    ay, by, cy = py[1] - py[0], py[2] - py[0], py[0] - py[1] - py[2] + py[3]
    u, v = np.full(x.shape, 0.5), np.full(x.shape, 0.5)
    for _ in range(iterations):
        fx = px[0] + ax * u + bx * v + cx * u * v - x
        fy = py[0] + ay * u + by * v + cy * u * v - y
        j11, j12, j21, j22 = ax + cx * v, bx + cx * u, ay + cy * v, by + cy * u
        det = j11 * j22 - j12 * j21
        u, v = u - (j22 * fx - j12 * fy) / det, v - (j11 * fy - j21 * fx) / det
    uc, vc = np.clip(u, 0, 1), np.clip(v, 0, 1)
    out[m] = pv[0] * (1 - uc) * (1 - vc) + pv[1] * uc * (1 - vc) + pv[2] * (1 - uc) * vc + pv[3] * uc * vc
    uu[m], vv[m] = u, v
    return out, uu, vv


# ---- the case list -------------------------------------------------------------------------------------------------------------------------
CARTESIAN, GEODETIC = 1, 0      # gridpp.Cartesian / gridpp.Geodetic (include/gridpp.h CoordinateType)
MESHES = {
    "metres": (lambda: warped_metres(31, 37, 3), CARTESIAN),
    "metres_6e5": (lambda: warped_metres(31, 37, 5, 6e5, -4e5), CARTESIAN),
    "metres_7e6": (lambda: warped_metres(31, 37, 7, 7e6, 5e6), CARTESIAN),
    "degrees": (lambda: warped_degrees(31, 37, 4), GEODETIC),
    "trapezoid0": (lambda: trapezoid(17, 19, 0), CARTESIAN),
    "trapezoid1": (lambda: trapezoid(17, 19, 1), CARTESIAN),
}
NQ = 4000
CASE_IDS = ["%s-%s" % (m, o) for m in MESHES for o in ORIENTATIONS]


def family(case_id):
    m = case_id.split("-")[0]
    return "metres" if m.startswith("metres") else m.rstrip("01")


class GeneralCase:
    """one mesh in one orientation, its 4000 queries and two fields; everything float32 as the library stores it"""

    def __init__(self, case_id):
        mesh, how = case_id.split("-")
        build, self.ctype = MESHES[mesh]
        lats, lons = orient(*build(), how)
        self.id, self.family = case_id, family(case_id)
        self.lats, self.lons = np.ascontiguousarray(lats, F32), np.ascontiguousarray(lons, F32)
        self.shape = self.lats.shape
        seed = CASE_IDS.index(case_id)
        self.qlat, self.qlon = queries(self.lats, self.lons, NQ, 100 + seed)
        self.values = np.random.default_rng(200 + seed).normal(0, 3, self.shape).astype(F32)
        # a field linear in (lon, lat) with a range of 5: any bilinear patch reproduces it
        self.lin = lambda y, x: (2.0 * (np.asarray(x, F64) - F64(self.lons.min())) / F64(np.ptp(self.lons.astype(F64)))   # noqa: E731
                                 + 3.0 * (np.asarray(y, F64) - F64(self.lats.min())) / F64(np.ptp(self.lats.astype(F64))))
        self.linear = self.lin(self.lats, self.lons).astype(F32)

    # -- the oracle's side, computed once per process and left unchanged --
    @functools.cached_property
    def opts(self):
        from oracle import oracle as O
        return O.Pts(self.lats.ravel(), self.lons.ravel(), ctype=self.ctype), O.Pts(self.qlat, self.qlon, ctype=self.ctype)

    @functools.cached_property
    def boxes(self):
        """oracle.get_box for every query -> (n, 5) int32: inside, Y1, X1, Y2, X2"""
        return oracle_boxes(self.lats, self.lons, self.qlat, self.qlon, self.ctype)

    @functools.cached_property
    def nearest(self):
        from oracle import oracle as O
        return O.nearest(*self.opts, self.values)

    def oracle(self, values):
        from oracle import oracle as O
        return O.bilinear(self.opts[0], self.shape, self.opts[1], values)

    @functools.cached_property
    def oracle_values(self):
        return self.oracle(self.values)

    @functools.cached_property
    def oracle_linear(self):
        return self.oracle(self.linear)

    @functools.cached_property
    def truth_values(self):
        return truth(self.lats, self.lons, self.values, self.boxes, self.qlat, self.qlon)

    @functools.cached_property
    def truth_linear(self):
        return truth(self.lats, self.lons, self.linear, self.boxes, self.qlat, self.qlon)[0]

    @functools.cached_property
    def roots(self):
        """root_taken for the queries with a box -> (alpha_first, beta_first, has_alpha, has_beta)"""
        m = self.boxes[:, 0] != 0
        Y1, X1, Y2, X2 = (self.boxes[m, k] for k in range(1, 5))
        xs = tuple(self.lons[k] for k in ((Y1, X1), (Y2, X1), (Y1, X2), (Y2, X2)))
        ys = tuple(self.lats[k] for k in ((Y1, X1), (Y2, X1), (Y1, X2), (Y2, X2)))
        return root_taken(xs, ys, self.qlon[m], self.qlat[m])


@functools.lru_cache(maxsize=None)
def case(case_id):
    return GeneralCase(case_id)


def oracle_boxes(lats, lons, qlat, qlon, ctype):
    """the oracle's get_box for many queries: one batched nearest-neighbour search, then the box search per query"""
    import ctypes as C
    from oracle import oracle as O
    la, lo = np.ascontiguousarray(lats, F32), np.ascontiguousarray(lons, F32)
    qlat, qlon = np.ascontiguousarray(qlat, F32), np.ascontiguousarray(qlon, F32)
    nY, nX = la.shape
    out = np.full((qlat.size, 5), -1, np.int32)
    out[:, 0] = 0
    if la.size == 0:
        return out
    nn = O.nearest_indices(O.Pts(la.ravel(), lo.ravel(), ctype=ctype), O.Pts(qlat, qlon, ctype=ctype))
    f = O.lib().orc_get_box
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float] + [C.POINTER(C.c_int)] * 4
    box = (C.c_int * 4)()
    ptrs = [C.cast(C.byref(box, 4 * k), C.POINTER(C.c_int)) for k in range(4)]
    for i in range(qlat.size):
        out[i, 0] = f(la.ctypes.data, lo.ctypes.data, nY, nX, int(nn[i]), float(qlat[i]), float(qlon[i]), *ptrs)
        out[i, 1:] = box[:]
    return out


# ---- grids of height or width 1 or 2 ------------------------------------------------------------------------------------------------------
DEGENERATE_SHAPES = ((1, 5), (5, 1), (1, 1), (2, 2), (2, 5), (5, 2))


@functools.lru_cache(maxsize=None)
def degenerate(shape):
    """the axis-0 trapezoid rule at a tiny shape with a node, an interior point, the centre, the far corner and a point outside
    -> dict(lats, lons, values, qlat, qlon, expected = the oracle's bilinear, nearest = the oracle's nearest)"""
    from oracle import oracle as O
    Y, X = shape
    lats, lons = (np.ascontiguousarray(a, F32) for a in trapezoid(Y, X, 0))
    la, lo = lats.astype(F64), lons.astype(F64)
    values = (1 + np.arange(Y * X, dtype=F32).reshape(Y, X) * F32(1.5)) ** 2
    qlat = np.array([la[0, 0], 0.3 * la.min() + 0.7 * la.max() + 0.01, (la.min() + la.max()) / 2, la[-1, -1], la.max() + 3], F32)
    qlon = np.array([lo[0, 0], 0.6 * lo[0].min() + 0.4 * lo[0].max() + 0.01, (lo.min() + lo.max()) / 2, lo[-1, -1], lo.max() + 3], F32)
    g, q = O.Pts(lats.ravel(), lons.ravel(), ctype=CARTESIAN), O.Pts(qlat, qlon, ctype=CARTESIAN)
    return dict(lats=lats, lons=lons, values=values, qlat=qlat, qlon=qlon, expected=O.bilinear(g, shape, q, values),
                nearest=O.nearest(g, q, values), boxes=oracle_boxes(lats, lons, qlat, qlon, CARTESIAN))
