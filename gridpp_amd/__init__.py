"""gridpp_amd -- the python surface of the MI355X-native gridpp hot path.

Mirrors the SWIG module of the reference (swig/gridpp.i %include "gridpp.h"):
same names, argument order, defaults, output dtypes (np.float32 / np.int32) and
exception mapping (ValueError for invalid arguments, RuntimeError otherwise), for
the optimal-interpolation + neighbourhood path only.  Use as

    import gridpp_amd as gridpp

All compute goes through libgridpp_hip.so (include/gridpp_hip.h).  Field
arguments may be anything numpy can convert (host path: staged through HBM by the
library) or torch CUDA tensors (device path: the kernels read/write the tensors'
HBM directly and a torch tensor is returned).
"""
import collections
import ctypes as C

import numpy as np

from . import _capi
from . import _marshal as _m
from ._capi import check, lib
from ._marshal import _empty_like_field, _host_empty, _is_dev, _mem, _ndim, _out_shape, _ptr, _shape, _vec, _wants_f64

__version__ = "0.8.0.dev1+mi355x.r1"

# include/gridpp.h:120-123, :88-100
Geodetic, Cartesian = 0, 1
Mean, Min, Median, Max, Quantile, Std, Variance, Sum, Count, RandomChoice, Unknown = 0, 10, 20, 30, 40, 50, 60, 70, 80, 90, -1
MV = np.nan
radius_earth = 6.378137e6


def version():
    return lib().gpp_version().decode()


def set_device(index):
    """One process per GPU: call with LOCAL_RANK before anything else."""
    check(lib().gpp_set_device(int(index)))


def device_count():
    n = C.c_int(0)
    check(lib().gpp_device_count(C.byref(n)))
    return n.value


def synchronize():
    check(lib().gpp_synchronize())


def is_valid(value):
    """src/api/util.cpp:16-18"""
    v = np.float32(value)
    return bool(not np.isnan(v) and not np.isinf(v))


def is_valid_lat(lat, type):
    """src/api/util.cpp:617-621: a Cartesian y is any valid value; a latitude lies within +-90.001 (the float against the double bound)"""
    if type == Cartesian:
        return is_valid(lat)
    return bool(is_valid(lat) and float(np.float32(lat)) >= -90.001 and float(np.float32(lat)) <= 90.001)


def is_valid_lon(lon, type):
    """src/api/util.cpp:622-624: any valid value, for both coordinate types"""
    return is_valid(lon)


def num_missing_values(array):
    """src/api/util.cpp:217-225: how many values of a 2-D array are NaN or infinite"""
    a = _vec(array, 2, "array")
    return int(a.size - np.count_nonzero(np.isfinite(a)))


# src/api/util.cpp:475-504
def init_vec2(Y, X, value=MV):
    return np.full((int(Y), int(X)), value, np.float32)


def init_ivec2(Y, X, value):
    return np.full((int(Y), int(X)), value, np.int32)


def init_vec3(Y, X, T, value=MV):
    return np.full((int(Y), int(X), int(T)), value, np.float32)


def init_ivec3(Y, X, T, value):
    return np.full((int(Y), int(X), int(T)), value, np.int32)


def compatible_size(a, b):
    """The seven overloads of src/api/util.cpp:427-474: (Grid, vec2), (Grid, vec3), (Points, vec), (Points, vec2), (vec2, vec2),
    (vec2, vec3) and (vec3, vec3).  A Grid or Points first argument decides the overload, then the rank of the arrays; an array
    without elements counts as one of the rank the overload asks for (numpy cannot tell [] from [[]])."""
    sb = np.shape(b)
    empty_b = 0 in sb
    if isinstance(a, Grid):
        if len(sb) not in (2, 3) and not empty_b:
            raise TypeError("compatible_size(Grid, v): v must have 2 or 3 dimensions")
        if sb[0] == 0:
            return True
        if len(sb) == 2:
            return a.size()[0] == sb[0] and a.size()[1] == sb[1]
        return sb[1] == 0 or (a.size()[0] == sb[1] and a.size()[1] == sb[2])   # v is [T][Y][X]; a v[0] without rows passes (:431)
    if isinstance(a, Points):
        if len(sb) == 1:
            return a.size() == sb[0]
        if len(sb) != 2:
            raise TypeError("compatible_size(Points, v): v must have 1 or 2 dimensions")
        return sb[0] == 0 or a.size() == sb[1]
    sa = np.shape(a)
    if (len(sa), len(sb)) == (2, 3):   # the first two sizes only (:448-461)
        return sa[0] == sb[0] and (sa[0] == 0 or sa[1] == sb[1])
    if len(sa) == len(sb) and len(sa) in (2, 3):
        return sa == sb
    if 0 in sa and empty_b:   # e.g. ([], [[]]): as far as both have sizes
        n = min(len(sa), len(sb))
        return sa[:n] == sb[:n]
    raise TypeError("compatible_size: no overload for arrays of %d and %d dimensions" % (len(sa), len(sb)))


_omp_threads = 1


def get_statistic(name):
    """gridpp::get_statistic (include/gridpp.h:1410, src/api/gridpp.cpp:11-43): the Statistic of a name.  The reference's table has no
    "variance": that name, like any other it does not know, gives Unknown."""
    return {"mean": Mean, "min": Min, "max": Max, "median": Median, "quantile": Quantile, "std": Std, "sum": Sum, "count": Count,
            "randomchoice": RandomChoice}.get(name, Unknown)


def set_omp_threads(num):   # src/api/gridpp.cpp:184-207 -- meaningless on the GPU path, kept for drop-in
    global _omp_threads
    _omp_threads = int(num)


def get_omp_threads():
    return _omp_threads


# ---- messages (include/gridpp.h:1394-1430, src/api/gridpp.cpp:70-76, src/api/util.cpp:226-252) ------------
_debug_level = 0


def set_debug_level(level):
    global _debug_level
    _debug_level = int(level)


def get_debug_level():
    return _debug_level


def debug(string):
    print(string, flush=True)


def warning(string):
    print("Warning: " + str(string), flush=True)


def error(string):
    print("Error: " + str(string), flush=True)
    raise RuntimeError(string)


def future_deprecation_warning(function, other=""):
    print("Future deprecation warning: %s will be deprecated%s" % (function, (", use %s instead." % other) if other else "."), flush=True)


def clock():
    """seconds since the epoch (src/api/util.cpp:254-260)"""
    import time
    return time.time()


# ---- Point / KDTree / Points / Grid -----------------------------------------------------------
class Point:
    """include/gridpp.h:1713-1743, src/api/point.cpp:5-26"""

    def __init__(self, lat, lon, elev=MV, laf=MV, type=Geodetic, x=None, y=None, z=None):
        self.lat, self.lon, self.elev, self.laf, self.type = float(lat), float(lon), float(elev), float(laf), type
        if x is not None:
            self.x, self.y, self.z = float(x), float(y), float(z)
        elif type == Geodetic:
            xs, ys, zs = convert_coordinates([lat], [lon], type)
            self.x, self.y, self.z = float(xs[0]), float(ys[0]), float(zs[0])
        else:   # point.cpp:18-21 (x = lat, y = lon)
            self.x, self.y, self.z = float(np.float32(lat)), float(np.float32(lon)), 0.0

    def _seven(self):
        return (C.c_float * 7)(self.x, self.y, self.z, self.elev, self.laf, self.lat, self.lon)


def convert_coordinates(lats, lons, type=Geodetic):
    """src/api/util.cpp:583-615; the scalar overload (:617-633) returns (ok, x, y, z)"""
    if np.isscalar(lats) and np.isscalar(lons):
        x, y, z = convert_coordinates([lats], [lons], type)
        return True, float(x[0]), float(y[0]), float(z[0])
    lats, lons = _vec(lats, 1, "lats"), _vec(lons, 1, "lons")
    if lats.size != lons.size:
        raise ValueError("lats and lons must have the same size")
    n = lats.size
    x, y, z = (np.empty(n, np.float32) for _ in range(3))
    check(lib().gpp_convert_coordinates(_ptr(lats), _ptr(lons), n, type, _ptr(x), _ptr(y), _ptr(z)))
    return x, y, z


def _is_big_f64(*arrays):
    """float64 numpy coordinate arrays of a large set: handed to the C-ABI as they are and cast to float32 on the device
    (numpy's astype on 16 M doubles takes longer than building the whole Grid)"""
    return all(isinstance(a, np.ndarray) and a.dtype == np.float64 for a in arrays) and arrays[0].size >= (1 << 16)


class _PointSet:
    """Owns a gpp_points handle (x/y/z resident in HBM)."""
    _h = None

    def __del__(self):
        try:
            if self._h is not None:
                lib().gpp_points_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _field(self, k):
        out = np.empty(self._n, np.float32)
        check(lib().gpp_points_get(self._h, k, _ptr(out)))
        return out

    def get_coordinate_type(self):
        return self._type

    # KDTree queries (src/api/kdtree.cpp:18-106)
    def _neighbours(self, lat, lon, radius, include_match=True, want_dist=False):
        cap = max(self._n, 1)
        idx = np.empty(cap, np.int32)
        dist = np.empty(cap, np.float32) if want_dist else None
        cnt = C.c_int(0)
        check(lib().gpp_points_get_neighbours(self._h, float(lat), float(lon), float(radius), int(bool(include_match)),
                                              _ptr(idx), _ptr(dist), cap, C.byref(cnt)))
        if want_dist:
            return idx[:cnt.value].copy(), dist[:cnt.value].copy()
        return idx[:cnt.value].copy()

    def _closest(self, lat, lon, num, include_match=True):
        idx = np.empty(max(int(num), 1), np.int32)
        cnt = C.c_int(0)
        check(lib().gpp_points_get_closest_neighbours(self._h, float(lat), float(lon), int(num), int(bool(include_match)),
                                                      _ptr(idx), C.byref(cnt)))
        return idx[:cnt.value].copy()

    def _nearest_flat(self, lats, lons, include_match=True):
        lats, lons = _vec(lats, 1), _vec(lons, 1)
        out = np.empty(lats.size, np.int32)
        check(lib().gpp_points_nearest_neighbour(self._h, _ptr(lats), _ptr(lons), lats.size, int(bool(include_match)), _ptr(out)))
        return out


class Points(_PointSet):
    """include/gridpp.h:1876-1968, src/api/points.cpp"""

    def __init__(self, lats=(), lons=(), elevs=(), lafs=(), type=Geodetic):
        f64 = _is_big_f64(lats, lons)
        lats, lons = _m.field(lats, 1, "lats", f64), _m.field(lons, 1, "lons", f64)
        elevs, lafs = _m.field(elevs, 1, "elevs", f64), _m.field(lafs, 1, "lafs", f64)
        n = lats.size
        if lons.size != n:
            raise ValueError("Cannot create points with unequal lat and lon sizes")
        if elevs.size not in (0, n):
            raise ValueError("'elevs' must either be size 0 or the same size at lats/lons")
        if lafs.size not in (0, n):
            raise ValueError("'lafs' must either be size 0 or the same size at lats/lons")
        h = C.c_void_p()
        create = lib().gpp_points_create_f64 if f64 else lib().gpp_points_create
        check(create(_ptr(lats), _ptr(lons), _ptr(elevs) if elevs.size == n and n else None,
                     _ptr(lafs) if lafs.size == n and n else None, n, type, C.byref(h)))
        self._h, self._n, self._type = h, n, type

    def size(self):
        return self._n

    def get_lats(self):
        return self._field(0)

    def get_lons(self):
        return self._field(1)

    def get_elevs(self):
        return self._field(2)

    def get_lafs(self):
        return self._field(3)

    def get_neighbours(self, lat, lon, radius, include_match=True):
        return self._neighbours(lat, lon, radius, include_match)

    def get_neighbours_with_distance(self, lat, lon, radius, include_match=True):
        return self._neighbours(lat, lon, radius, include_match, True)

    def get_num_neighbours(self, lat, lon, radius, include_match=True):
        return len(self._neighbours(lat, lon, radius, include_match))

    def get_nearest_neighbour(self, lat, lon, include_match=True):
        return int(self._nearest_flat([lat], [lon], include_match)[0])

    def get_closest_neighbours(self, lat, lon, num, include_match=True):
        return self._closest(lat, lon, num, include_match)

    def get_point(self, index):   # src/api/points.cpp:128-130
        f = [self._field(k)[index] for k in range(7)]
        return Point(f[0], f[1], f[2], f[3], self._type, f[4], f[5], f[6])

    def get_in_domain_indices(self, grid):   # src/api/points.cpp:77-92: the points some grid box encloses (Grid::get_box)
        if self._n == 0 or grid._n == 0:
            return np.zeros(0, np.int32)
        lats, lons = np.ascontiguousarray(self.get_lats(), np.float32), np.ascontiguousarray(self.get_lons(), np.float32)
        inside, boxes = np.zeros(self._n, np.int32), np.zeros(4 * self._n, np.int32)
        check(lib().gpp_grid_get_box(grid._h, _ptr(lats), _ptr(lons), self._n, _ptr(inside), _ptr(boxes)))
        return np.nonzero(inside)[0].astype(np.int32)

    def get_in_domain(self, grid):           # points.cpp:93-109 (the new set is built with the default coordinate type)
        idx = self.get_in_domain_indices(grid)
        return Points(self.get_lats()[idx], self.get_lons()[idx], self.get_elevs()[idx], self.get_lafs()[idx])

    def subset(self, indices):
        indices = np.asarray(indices, np.int64)
        if indices.size and indices.max() >= self._n:
            raise ValueError("Index exceeds number of points")
        return Points(self.get_lats()[indices], self.get_lons()[indices], self.get_elevs()[indices], self.get_lafs()[indices])


class KDTree(Points):
    """include/gridpp.h:1746-1873 (a Points without elev/laf)"""

    def __init__(self, lats=(), lons=(), type=Geodetic):
        Points.__init__(self, lats, lons, (), (), type)

    # static distance helpers (src/api/kdtree.cpp:107-200); host scalar math like the reference's
    @staticmethod
    def calc_straight_distance(*args):
        """(p1, p2) or (x0, y0, z0, x1, y1, z1): 3-D chord length in float32 (kdtree.cpp:189-194)"""
        if len(args) == 2:
            p1, p2 = args
            args = (p1.x, p1.y, p1.z, p2.x, p2.y, p2.z)
        f = np.float32
        x0, y0, z0, x1, y1, z1 = (f(a) for a in args)
        return float(np.sqrt((x0 - x1) * (x0 - x1) + (y0 - y1) * (y0 - y1) + (z0 - z1) * (z0 - z1), dtype=np.float32))

    @staticmethod
    def deg2rad(deg):
        return float(np.float32(np.float64(np.float32(deg)) * np.pi / 180))

    @staticmethod
    def rad2deg(rad):
        return float(np.float32(np.float64(np.float32(rad)) * 180 / np.pi))

    @staticmethod
    def calc_distance(*args):
        """(p1, p2) or (lat1, lon1, lat2, lon2, type=Geodetic): great-circle distance (kdtree.cpp:107-136,182-187)"""
        if len(args) == 2:
            p1, p2 = args
            if p1.type != p2.type:
                raise RuntimeError("Coordinate types must be the same")
            args = (p1.lat, p1.lon, p2.lat, p2.lon, p1.type)
        lat1, lon1, lat2, lon2 = (np.float32(a) for a in args[:4])
        ctype = args[4] if len(args) > 4 else Geodetic
        if ctype == Cartesian:
            dx, dy = lon1 - lon2, lat1 - lat2
            return float(np.sqrt(dx * dx + dy * dy, dtype=np.float32))
        if lat1 == lat2 and lon1 == lon2:
            return 0.0
        r = [np.float64(np.float32(np.float64(v) * np.pi / 180)) for v in (lat1, lat2, lon1, lon2)]   # deg2rad returns float
        lat1r, lat2r, lon1r, lon2r = r
        ratio = (np.cos(lat1r) * np.cos(lon1r) * np.cos(lat2r) * np.cos(lon2r) + np.cos(lat1r) * np.sin(lon1r) * np.cos(lat2r) * np.sin(lon2r)
                 + np.sin(lat1r) * np.sin(lat2r))
        return float(np.float32(np.arccos(ratio) * 6.378137e6))

    @staticmethod
    def calc_distance_fast(*args):
        """(p1, p2) or (lat1, lon1, lat2, lon2, type=Geodetic): equirectangular approximation (kdtree.cpp:137-181)"""
        if len(args) == 2:
            p1, p2 = args
            args = (p1.lat, p1.lon, p2.lat, p2.lon, p1.type)
        lat1, lon1, lat2, lon2 = (np.float32(a) for a in args[:4])
        ctype = args[4] if len(args) > 4 else Geodetic
        if ctype == Cartesian:
            dx, dy = lon1 - lon2, lat1 - lat2
            return float(np.sqrt(dx * dx + dy * dy, dtype=np.float32))
        lat1r, lat2r, lon1r, lon2r = [np.float64(np.float32(np.float64(v) * np.pi / 180)) for v in (lat1, lat2, lon1, lon2)]
        dlon = np.fmod(np.abs(lon1r - lon2r), 2 * np.pi)
        if dlon > np.pi:
            dlon = 2 * np.pi - dlon
        max_lat = lat2r if np.abs(lat2r) > np.abs(lat1r) else lat1r
        dx2 = np.float32(np.cos(max_lat) ** 2 * dlon * dlon)
        dy2 = np.float32((lat1r - lat2r) * (lat1r - lat2r))
        return float(np.float32(6.378137e6 * np.sqrt(np.float64(dx2 + dy2))))


# SWIG's flat names of the static KDTree methods (the reference's tests use them: tests/test_kdtree.py:56-58,111-112)
KDTree_calc_distance = KDTree.calc_distance
KDTree_calc_distance_fast = KDTree.calc_distance_fast
KDTree_calc_straight_distance = KDTree.calc_straight_distance
KDTree_deg2rad = KDTree.deg2rad
KDTree_rad2deg = KDTree.rad2deg


class Grid(_PointSet):
    """include/gridpp.h:1971-2060, src/api/grid.cpp"""

    def __init__(self, lats=((),), lons=((),), elevs=((),), lafs=((),), type=Geodetic):
        f64 = _is_big_f64(lats, lons)
        lats, lons = _m.field(lats, 2, "lats", f64), _m.field(lons, 2, "lons", f64)
        elevs, lafs = _m.field(elevs, 2, "elevs", f64), _m.field(lafs, 2, "lafs", f64)
        if lats.shape != lons.shape:
            raise ValueError("lats and lons must have the same shape")
        ny, nx = lats.shape
        if ny * nx == 0:
            ny = nx = 0
        e = elevs if elevs.shape == lats.shape and elevs.size else None   # grid.cpp:41-54
        l = lafs if lafs.shape == lats.shape and lafs.size else None
        h = C.c_void_p()
        create = lib().gpp_grid_create_f64 if f64 else lib().gpp_grid_create
        check(create(_ptr(lats), _ptr(lons), _ptr(e), _ptr(l), ny, nx, type, C.byref(h)))
        self._h, self._n, self._ny, self._nx, self._type = h, ny * nx, ny, nx, type

    def size(self):
        return [self._ny, self._nx]

    def _f2(self, k):
        return self._field(k).reshape(self._ny, self._nx)

    def get_lats(self):
        return self._f2(0)

    def get_lons(self):
        return self._f2(1)

    def get_elevs(self):
        return self._f2(2)

    def get_lafs(self):
        return self._f2(3)

    def get_nearest_neighbour(self, lat, lon, include_match=True):   # grid.cpp:76-82,108-114
        if self._n == 0:
            return []
        i = int(self._nearest_flat([lat], [lon], include_match)[0])
        return [i // self._nx, i % self._nx]

    def get_neighbours(self, lat, lon, radius, include_match=True):
        idx = self._neighbours(lat, lon, radius, include_match)
        return np.stack([idx // self._nx, idx % self._nx], axis=1).astype(np.int32) if idx.size else np.zeros((0, 2), np.int32)

    def get_closest_neighbours(self, lat, lon, num, include_match=True):   # grid.cpp:72-75
        idx = self._closest(lat, lon, num, include_match)
        return np.stack([idx // self._nx, idx % self._nx], axis=1).astype(np.int32) if idx.size else np.zeros((0, 2), np.int32)

    def get_num_neighbours(self, lat, lon, radius, include_match=True):
        return len(self._neighbours(lat, lon, radius, include_match))

    def get_neighbours_with_distance(self, lat, lon, radius, include_match=True):   # grid.cpp:62-66
        idx, dist = self._neighbours(lat, lon, radius, include_match, True)
        ij = np.stack([idx // self._nx, idx % self._nx], axis=1).astype(np.int32) if idx.size else np.zeros((0, 2), np.int32)
        return ij, dist

    def get_point(self, y_index, x_index):   # grid.cpp:230-233
        i = int(y_index) * self._nx + int(x_index)
        f = [self._field(k)[i] for k in range(7)]
        return Point(f[0], f[1], f[2], f[3], self._type, f[4], f[5], f[6])

    def get_box(self, lat, lon):   # grid.cpp:149-229 -> [inside, Y1, X1, Y2, X2] (swig/gridpp.i:73-76 OUTPUT ints)
        qlat, qlon = np.array([lat], np.float32), np.array([lon], np.float32)
        inside, box = np.zeros(1, np.int32), np.zeros(4, np.int32)
        check(lib().gpp_grid_get_box(self._h, _ptr(qlat), _ptr(qlon), 1, _ptr(inside), _ptr(box)))
        return [bool(inside[0])] + [int(b) for b in box]

    def to_points(self):   # grid.cpp:131-145
        return Points(self._field(0), self._field(1), self._field(2), self._field(3), self._type)


# ---- structure functions (include/gridpp.h:2069-2343, src/api/structure.cpp) -----------------------
_SK = dict(Barnes=0, Cressman=1, Soar=2, Toar=3, Powerlaw=4, Linear=5)
_ST_HAS_LOC, _ST_CV = 1, 2


class StructureFunction:
    """Base of the scalar structure functions; owns the gpp_structure descriptor handed to the C-ABI."""
    _s = None

    def _copy_struct(self):
        t = _capi.gpp_structure()
        C.memmove(C.byref(t), C.byref(self._s), C.sizeof(t))
        return t

    def localization_distance(self, p=None):
        d = C.c_float(0)
        lat, lon = (p.lat, p.lon) if p is not None else (0.0, 0.0)
        if p is None and self._s.field:
            raise ValueError("a spatially varying structure needs the point")
        check(lib().gpp_structure_localization_distance(C.byref(self._s), float(lat), float(lon), C.byref(d)))
        return d.value

    def _corr(self, p1, p2, background, device=None):
        """corr / corr_background of p1 against one Point (a float), a list or tuple of Points (np.float32 array) or every point of a
        Points / KDTree / Grid (an array shaped like it; a torch tensor on `device` if one is given): the scales of a spatially varying
        structure are looked up at p1 once and all pairs run in one launch (structure.cpp:231-267)"""
        if isinstance(p2, _PointSet):
            shape = _out_shape(p2)
            if device is None:
                out = _host_empty(shape)
                mem = _capi.MEM_HOST
            else:
                import torch
                out = torch.empty(shape, dtype=torch.float32, device=device)
                if not _is_dev(out):
                    raise ValueError("device must be a GPU device")
                mem = _capi.MEM_DEVICE
            check(lib().gpp_structure_corr_points(C.byref(self._s), p1._seven(), p2._h, int(background), _ptr(out), mem))
            return out
        if isinstance(p2, (list, tuple)):
            rec = np.array([(q.x, q.y, q.z, q.elev, q.laf, q.lat, q.lon) for q in p2], np.float32).reshape(len(p2), 7)
            out = np.empty(len(p2), np.float32)
            check(lib().gpp_structure_corr_many(C.byref(self._s), p1._seven(), _ptr(rec), len(p2), int(background), _ptr(out)))
            return out
        r = C.c_float(0)
        check(lib().gpp_structure_corr(C.byref(self._s), p1._seven(), p2._seven(), int(background), C.byref(r)))
        return r.value

    def corr(self, p1, p2, device=None):
        return self._corr(p1, p2, 0, device)

    def corr_background(self, p1, p2, device=None):
        return self._corr(p1, p2, 1, device)

    def clone(self):
        c = StructureFunction.__new__(type(self))
        c._s = self._copy_struct()
        c._field_owner = getattr(self, "_field_owner", None)   # keeps the HBM fields (and their grid) alive
        return c


class _Field:
    """Owns a gpp_field (h, v, w fields of a spatially varying structure resident in HBM)."""

    def __init__(self, grid, h, v, w, kind, min_rho):
        self.grid = grid   # the field borrows the grid handle
        self.h = C.c_void_p()
        check(lib().gpp_field_create(grid._h, _ptr(h), _ptr(v), _ptr(w), kind, float(min_rho), C.byref(self.h)))

    def __del__(self):
        try:
            if self.h:
                lib().gpp_field_destroy(self.h)
                self.h = None
        except Exception:
            pass


def _scalar_structure(obj, kind, h, v, w, hmax):
    if isinstance(h, Grid):   # (grid, h, v, w, min_rho): spatially varying form, e.g. src/api/structure.cpp:168-184
        grid, hf, vf, wf = h, v, w, hmax
        raise RuntimeError("internal: use _spatial_structure")
    for name, val in (("v", v), ("w", w)):   # e.g. structure.cpp:147-152
        if not is_valid(val) or val < 0:
            raise ValueError("%s must be >= 0" % name)
    mr = C.c_float(0)
    check(lib().gpp_structure_min_rho(kind, float(h), float(hmax), C.byref(mr)))
    obj._s = _capi.gpp_structure(kind, float(h), float(v), float(w), mr.value, 0, 0, 0.0, 0.0, 0, None)


def _spatial_structure(obj, kind, grid, h, v, w, min_rho):
    h, v, w = _m.field(h, 2, "h"), _m.field(v, 2, "v"), _m.field(w, 2, "w")
    if h.shape == (1, 1) and v.shape == (1, 1) and w.shape == (1, 1):   # not spatial (structure.cpp:174-176)
        obj._s = _capi.gpp_structure(kind, float(h[0, 0]), float(v[0, 0]), float(w[0, 0]), float(min_rho), 0, 0, 0.0, 0.0, 0, None)
        return
    shape = tuple(grid.size())
    if h.shape != shape or v.shape != shape or w.shape != shape:
        raise ValueError("Grid size not the same as scale size")
    obj._field_owner = _Field(grid, h, v, w, kind, min_rho)
    obj._s = _capi.gpp_structure(kind, 0.0, 0.0, 0.0, float(min_rho), 0, 0, 0.0, 0.0, 0, obj._field_owner.h)


def _make_structure(obj, kind, args, has_hmax=True):
    """(h, v=0, w=0, hmax=MV) or (grid, h, v, w, min_rho=0.0013)"""
    if len(args) and isinstance(args[0], Grid):
        if len(args) < 4:
            raise TypeError("spatially varying structure: (grid, h, v, w, min_rho=0.0013)")
        _spatial_structure(obj, kind, args[0], args[1], args[2], args[3], args[4] if len(args) > 4 else 0.0013)
    else:
        a = list(args) + [0, 0, MV][len(args) - 1:] if len(args) < 4 else list(args)
        _scalar_structure(obj, kind, a[0], a[1], a[2], a[3] if has_hmax else MV)


class BarnesStructure(StructureFunction):
    """BarnesStructure(h, v=0, w=0, hmax=MV) (src/api/structure.cpp:143-167)"""

    def __init__(self, *args):
        _make_structure(self, _SK["Barnes"], args)


class CressmanStructure(StructureFunction):
    """CressmanStructure(h, v=0, w=0) (src/api/structure.cpp:287-312)"""

    def __init__(self, h, v=0, w=0):
        if not is_valid(h) or h < 0:   # StructureFunction(localization_distance) base ctor, structure.cpp:7-12
            raise ValueError("Structure function initizlied with invalid localization distance")
        _scalar_structure(self, _SK["Cressman"], h, v, w, MV)


class SoarStructure(StructureFunction):
    def __init__(self, *args):   # structure.cpp:317-341
        _make_structure(self, _SK["Soar"], args)


class ToarStructure(StructureFunction):
    def __init__(self, *args):   # structure.cpp:467-491
        _make_structure(self, _SK["Toar"], args)


class PowerlawStructure(StructureFunction):
    def __init__(self, *args):   # structure.cpp:618-642
        _make_structure(self, _SK["Powerlaw"], args)


class LinearStructure(StructureFunction):
    def __init__(self, *args):   # structure.cpp:765-789
        _make_structure(self, _SK["Linear"], args)


class MultipleStructure(StructureFunction):
    """MultipleStructure(structure_h, structure_v, structure_w) (src/api/structure.cpp:90-138): the horizontal factor
    (and the localization distance) comes from structure_h, the vertical one from structure_v, the land-area-fraction
    one from structure_w."""

    def __init__(self, structure_h, structure_v, structure_w):
        sh, sv, sw = structure_h._s, structure_v._s, structure_w._s
        kv = sv.kind_v - 1 if sv.kind_v else sv.kind
        kw = sw.kind_w - 1 if sw.kind_w else sw.kind
        # A component may itself be a MultipleStructure (the reference simply delegates, structure.cpp:90-138): structure_h then
        # contributes its horizontal part, structure_v the vertical part of ITS vertical component (kind_v, v, field_v) and
        # structure_w the laf part of its laf component.
        # spatially varying parts: the horizontal scale (and the localization distance) from structure_h's field, the vertical
        # scale from structure_v's, the laf scale from structure_w's (each at the nearest point of ITS grid to the first point)
        self._field_owner = [getattr(t, "_field_owner", None) for t in (structure_h, structure_v, structure_w)]
        if sh.field:
            loc, flags = 0.0, 0
        else:
            loc, flags = structure_h.localization_distance(), _ST_HAS_LOC
        fv = sv.field_v if sv.kind_v else sv.field
        fw = sw.field_w if sw.kind_w else sw.field
        self._s = _capi.gpp_structure(sh.kind, sh.h, sv.v, sw.w, sh.min_rho, kv + 1, kw + 1, loc, 0.0, flags, sh.field, fv, fw)


class CrossValidation(StructureFunction):
    """CrossValidation(structure, dist) (src/api/structure.cpp:910-944)"""

    def __init__(self, structure, dist):
        if not is_valid(dist) or dist < 0:
            raise ValueError("Invalid 'dist' in CrossValidation structure")
        self._s = structure._copy_struct()
        self._s.flags |= _ST_CV
        self._s.cv_dist = float(dist)
        self._field_owner = getattr(structure, "_field_owner", None)


def _structure(s):
    if not isinstance(s, StructureFunction) or s._s is None:
        raise RuntimeError("structure must be one of the gridpp_amd structure functions")
    return C.byref(s._s)


# ---- optimal interpolation (include/gridpp.h:162-248, src/api/oi.cpp) -----------------------------
def _oi_common(bg, background, bvariance, points, pobs, obs_variance, pbackground, bvariance_at_points,
               structure, max_points, allow_extrapolation, want_variance, deferred=False):
    if max_points < 0:
        raise ValueError("max_points must be >= 0")
    if not isinstance(bg, (Grid, Points)) or not isinstance(points, Points):
        raise TypeError("bgrid must be a Grid or Points, points a Points")
    if bg.get_coordinate_type() != points.get_coordinate_type():
        raise ValueError("Both background and observations points must be of same coordinate type (lat/lon or x/y)")
    nd = 2 if isinstance(bg, Grid) else 1
    f64 = _wants_f64(background, bvariance)
    background = _m.field(background, nd, "background", f64)
    shape = _out_shape(bg)
    if _shape(background) != shape:
        raise ValueError("input field %s is not the same size as the grid %s" % (_shape(background), shape))
    bvariance = _m.field(bvariance, nd, "bvariance", f64)
    if bvariance is not None and _shape(bvariance) != shape:
        raise ValueError("Input bvariance is not the same size as the grid")
    S = points.size()
    pobs, obs_variance = _m.field(pobs, 1, "obs", f64), _m.field(obs_variance, 1, "variance", f64)
    pbackground = _m.field(pbackground, 1, "background_at_points", f64)
    for name, a in (("Observations", pobs), ("Ratios", obs_variance), ("Background", pbackground)):
        if _shape(a)[0] != S:
            raise ValueError("%s (%d) and points (%d) size mismatch" % (name, _shape(a)[0], S))
    bvariance_at_points = _m.field(bvariance_at_points, 1, "bvariance_at_points", f64)
    if bvariance_at_points is not None and _shape(bvariance_at_points)[0] != S:
        raise ValueError("Background variance and points size mismatch")
    mem = _m.flags(f64, background, bvariance, pobs, obs_variance, pbackground, bvariance_at_points)
    out = _empty_like_field(shape, background)
    var = _empty_like_field(shape, background) if want_variance else None
    if deferred:
        if mem != _capi.MEM_DEVICE:
            raise ValueError("optimal_interpolation_async takes device-resident fields (torch tensors on the GPU)")
        mem |= _capi.ASYNC
    rc = lib().gpp_optimal_interpolation_full(bg._h, _ptr(background), _ptr(bvariance), points._h, _ptr(pobs),
                                              _ptr(obs_variance), _ptr(pbackground), _ptr(bvariance_at_points),
                                              _structure(structure), int(max_points), int(bool(allow_extrapolation)),
                                              _ptr(out), _ptr(var), mem)
    if deferred:   # (the inputs, the handles and the structure stay referenced until the wait)
        # The library queues EVERY GPP_ASYNC call, also one that failed at submission (as a completed call that reports its error again): the
        # mirror keeps its queue aligned with that one -- the entry of a failed submission is simply dropped when it reaches the front.
        pending = PendingAnalysis(out, var, (bg, background, bvariance, points, pobs, obs_variance, pbackground, bvariance_at_points, structure))
        check(rc)
        return pending
    check(rc)
    return out, var


class PendingAnalysis:
    """An optimal_interpolation call that was enqueued with GPP_ASYNC (include/gridpp_hip.h: gpp_wait): wait() returns the analysis (and the
    variance, if asked for) once it is complete and raises what the call would have raised.  The library completes its deferred calls in
    order: waiting for a later one first completes the earlier ones."""
    _tls = None      # per thread: the library queues deferred calls per calling thread (gpp_wait completes the oldest one of ITS thread)

    @classmethod
    def _q(cls):
        import threading
        if cls._tls is None:
            cls._tls = threading.local()
        if not hasattr(cls._tls, "q"):
            cls._tls.q = []
        return cls._tls.q

    def __init__(self, out, var, keep):
        self._out, self._var, self._keep, self._rc, self._msg = out, var, keep, None, None
        self._queue = PendingAnalysis._q()      # (wait() from another thread than the one that made the call is an error of the caller)
        self._queue.append(self)

    def _complete_front(self):
        front = self._queue.pop(0)
        front._rc = lib().gpp_wait()
        front._msg = lib().gpp_last_error().decode("utf-8", "replace") if front._rc != _capi.GPP_OK else None
        front._stats = oi_last_stats() if front._rc == _capi.GPP_OK else None
        front._keep = None

    def wait(self):
        while self._rc is None:
            self._complete_front()
        if self._rc == _capi.GPP_EINVAL:
            raise ValueError(self._msg)
        if self._rc != _capi.GPP_OK:
            raise RuntimeError(self._msg)
        return self._out if self._var is None else (self._out, self._var)

    def stats(self):
        """gpp_oi_last_stats of THIS call (valid after wait())"""
        self.wait()
        return self._stats


def optimal_interpolation_async(bgrid, background, points, pobs, pratios, pbackground, structure, max_points, allow_extrapolation=True):
    """optimal_interpolation on device-resident fields without waiting for the result: returns a PendingAnalysis.  For a caller that streams
    analyses through one GPU (one per observation set; bench.py, gridpp_amd.dist): in the steady state of such a stream -- the same Grid and
    Points objects as the call before -- the library needs the host for nothing and the next call can be enqueued while this one runs.
    The tensors passed in must not be modified before wait() returns."""
    return _oi_common(bgrid, background, None, points, pobs, pratios, pbackground, None, structure, max_points, allow_extrapolation, False, deferred=True)


def optimal_interpolation(bgrid, background, points, pobs, pratios, pbackground, structure, max_points, allow_extrapolation=True):
    """gridpp::optimal_interpolation, Grid (src/api/oi.cpp:26-87) and Points (:89-136) overloads."""
    return _oi_common(bgrid, background, None, points, pobs, pratios, pbackground, None, structure, max_points,
                      allow_extrapolation, False)[0]


def optimal_interpolation_full_async(bgrid, background, bvariance, points, obs, obs_variance, background_at_points,
                                     bvariance_at_points, structure, max_points, allow_extrapolation=True):
    """optimal_interpolation_full without waiting for the result (see optimal_interpolation_async): PendingAnalysis.wait() returns
    (analysis, analysis_variance)."""
    return _oi_common(bgrid, background, bvariance, points, obs, obs_variance, background_at_points, bvariance_at_points, structure, max_points,
                      allow_extrapolation, True, deferred=True)


def optimal_interpolation_full(bgrid, background, bvariance, points, obs, obs_variance, background_at_points,
                               bvariance_at_points, structure, max_points, allow_extrapolation=True):
    """gridpp::optimal_interpolation_full (src/api/oi.cpp:138-412); returns (analysis, analysis_variance)."""
    out, var = _oi_common(bgrid, background, bvariance, points, obs, obs_variance, background_at_points,
                          bvariance_at_points, structure, max_points, allow_extrapolation, True)
    return out, var


# ---- the reusable OI gain (include/gridpp_hip.h: gpp_oi_gain_*; no counterpart in the reference) ------------------
class OiGain:
    """What optimal_interpolation_gain returns: for every background point the selected observations, their weights and w . g."""

    def __init__(self, handle, bgrid, stations, max_points):
        self._h, self._nd, self._shape, self._S, self.max_points = handle, (2 if isinstance(bgrid, Grid) else 1), _out_shape(bgrid), stations, max_points

    def __del__(self):
        try:
            self.release()
        except Exception:   # noqa: BLE001  (interpreter shutdown)
            pass

    def release(self):
        """gpp_oi_gain_destroy: returns the HBM the gain holds (`nbytes`); the gain cannot be used afterwards."""
        h, self._h = self._h, None
        if h:
            check(lib().gpp_oi_gain_destroy(h))

    def _handle(self):
        if not self._h:
            raise RuntimeError("the gain was released")
        return self._h

    def apply(self, background, pobs, pbackground, allow_extrapolation=True):
        """The analysis of a field, (Y, X) / (N,), or of a stack of E fields in gridpp's cube layout, (Y, X, E) / (N, E) with
        pbackground (S, E) and pobs (S,) or (S, E) -- the argument shapes of optimal_interpolation_ensi.  numpy in, numpy out; torch CUDA
        tensors in, a torch CUDA tensor out.  ValueError naming the lowest (field, station) where a usable station has an invalid pobs or
        pbackground."""
        h = self._handle()
        nd = _ndim(background)
        if nd not in (self._nd, self._nd + 1):
            raise RuntimeError("background must have %d or %d dimensions" % (self._nd, self._nd + 1))
        stack = nd == self._nd + 1
        f64 = _wants_f64(background)
        background = _m.field(background, nd, "background", f64)
        if _shape(background)[:self._nd] != self._shape:
            raise ValueError("input field %s is not the same size as the grid %s" % (_shape(background), self._shape))
        E = _shape(background)[-1] if stack else 1
        if E < 1:
            raise ValueError("background holds no fields")
        pobs = _m.field(pobs, None, "pobs", f64)
        pbackground = _m.field(pbackground, None, "pbackground", f64)
        S = self._S
        if _shape(pobs) not in ((S,), (S, E)):
            raise ValueError("Observations %s and points (%d), fields (%d) size mismatch" % (_shape(pobs), S, E))
        if _shape(pbackground) != (S, E) and not (E == 1 and _shape(pbackground) == (S,)):
            raise ValueError("Background at points %s and points (%d), fields (%d) size mismatch" % (_shape(pbackground), S, E))
        per_field = int(len(_shape(pobs)) == 2 and E > 1)
        mem = _m.flags(f64, background, pobs, pbackground)
        out = _empty_like_field(_shape(background), background)
        check(lib().gpp_oi_gain_apply(h, _ptr(background), int(E), _ptr(pobs), per_field, _ptr(pbackground), int(bool(allow_extrapolation)),
                                      _ptr(out), mem))
        return out

    def analysis_variance(self, bvariance):
        """The analysis variance of optimal_interpolation_full for this background variance (with the gain's ratios)."""
        h = self._handle()
        bvariance = _m.field(bvariance, self._nd, "bvariance", False)
        if _shape(bvariance) != self._shape:
            raise ValueError("Input bvariance is not the same size as the grid")
        return _m.run(lib().gpp_oi_gain_variance, h, _ptr(bvariance), out_shape=self._shape, like=bvariance, mem=_m.flags(False, bvariance))

    def _info(self):
        cells, nbytes = C.c_longlong(), C.c_longlong()
        stations, mp, largest = C.c_int(), C.c_int(), C.c_int()
        check(lib().gpp_oi_gain_info(self._handle(), C.byref(cells), C.byref(stations), C.byref(mp), C.byref(nbytes), C.byref(largest)))
        return cells.value, stations.value, mp.value, nbytes.value, largest.value

    @property
    def nbytes(self):
        """HBM the gain holds now: about cells * max_points * 12 bytes plus 9 per cell (and the innovation table of its last apply)."""
        return self._info()[3]

    @property
    def largest_selection(self):
        return self._info()[4]

    def _selection(self, which):
        n = int(np.prod(self._shape))
        counts = np.empty(self._shape, np.int32) if which == 0 else None
        indices = np.empty(self._shape + (self.max_points,), np.int32) if which == 1 else None
        weights = np.empty(self._shape + (self.max_points,), np.float64) if which == 2 else None
        if n:
            check(lib().gpp_oi_gain_selection(self._handle(), _ptr(counts), _ptr(indices), _ptr(weights), _capi.MEM_HOST))
        return (counts, indices, weights)[which]

    def counts(self):
        """selected observations per background point: int32, the shape of a field"""
        return self._selection(0)

    def indices(self):
        """their indices into the observation arrays, ascending, -1 behind the selection: int32, field shape + (max_points,)"""
        return self._selection(1)

    def weights(self):
        """their weights w = G (P + R)^-1 (float64), 0 behind the selection: field shape + (max_points,)"""
        return self._selection(2)


def optimal_interpolation_gain(bgrid, points, pratios, structure, max_points, usable=None):
    """Everything of optimal_interpolation that does not depend on a value, computed once: which observations every background point
    selects (src/api/oi.cpp:229-287) and their weights (:304-317).  The returned OiGain analyses any number of fields with it --

        gain = optimal_interpolation_gain(grid, points, pratios, structure, 30)
        out = gain.apply(background, pobs, pbackground)          # = optimal_interpolation(grid, background, points, pobs, pratios, pbackground, structure, 30)
        out = gain.apply(background_yxe, pobs, pbackground_se)   # E fields in one call

    instead of a loop of optimal_interpolation calls over members, hours or perturbed observations with the same grid, stations,
    ratios, structure and max_points.  pratios is optimal_interpolation's; a caller of optimal_interpolation_full passes
    obs_variance / bvariance_at_points, divided in float32 as oi.cpp:194 does.  usable (S booleans, None: every station): the
    reference drops a station whose pobs or pbackground is missing in each call; a gain is told at construction which stations to
    leave out, and apply raises when a usable station has a missing value.  1 <= max_points <= 62.  The gain holds about
    cells * max_points * 12 bytes of HBM (5.9 GB for 4000 x 4000 points and max_points 30; `nbytes`) until release() / gpp_oi_gain_destroy
    or until it is garbage-collected."""
    if not isinstance(bgrid, (Grid, Points)) or not isinstance(points, Points):
        raise TypeError("bgrid must be a Grid or Points, points a Points")
    if bgrid.get_coordinate_type() != points.get_coordinate_type():
        raise ValueError("Both background and observations points must be of same coordinate type (lat/lon or x/y)")
    max_points = int(max_points)
    if max_points < 1:
        raise ValueError("max_points must be >= 1: a gain holds max_points columns per background point")
    if max_points > _capi.OI_GAIN_MAX_POINTS:
        raise ValueError("max_points must be <= %d (GPP_OI_GAIN_MAX_POINTS)" % _capi.OI_GAIN_MAX_POINTS)
    S = points.size()
    pratios = np.ascontiguousarray(np.asarray(pratios.cpu() if _is_dev(pratios) else pratios), dtype=np.float32)
    if pratios.ndim != 1 or pratios.shape[0] != S:
        raise ValueError("Ratios (%s) and points (%d) size mismatch" % (pratios.shape, S))
    if usable is not None:
        usable = np.ascontiguousarray(np.asarray(usable.cpu() if _is_dev(usable) else usable).astype(bool), dtype=np.uint8)
        if usable.ndim != 1 or usable.shape[0] != S:
            raise ValueError("usable (%s) and points (%d) size mismatch" % (usable.shape, S))
    handle = C.c_void_p()
    check(lib().gpp_oi_gain_create(bgrid._h, points._h, _ptr(pratios), _ptr(usable), _structure(structure), max_points, C.byref(handle)))
    return OiGain(handle, bgrid, S, max_points)


def oi_last_stats():
    s = _capi.gpp_oi_stats()
    check(lib().gpp_oi_last_stats(C.byref(s)))
    return dict(cells=s.cells, cells_updated=s.cells_updated, solves=s.solves, fallback_tiles=s.fallback_tiles, kernel_ms=s.kernel_ms,
                union_kernel_ms=s.union_kernel_ms, fallback_subtiles=s.fallback_subtiles, big_cells=s.big_cells, bulk_certified=s.bulk_certified,
                pair_window=s.pair_window, pair_table_bytes=s.pair_table_bytes, pair_fallback_items=s.pair_fallback_items, pair_table_build_ms=s.pair_table_build_ms)


def obs_index_axes(points):
    """Diagnostics: the two coordinate axes (0 = x, 1 = y, 2 = z) the observation index of `points` is binned on."""
    a, b = C.c_int(-1), C.c_int(-1)
    check(lib().gpp_debug_obs_axes(points._h, C.byref(a), C.byref(b)))
    return a.value, b.value


def obs_index_layout(points):
    """Diagnostics: the bin layout of the observation index of `points`: nbx, nby, amin, bmin, inv_s, bin_start [nbx * nby + 1] and
    whether the index was built on the device."""
    dims, geom = np.zeros(3, np.int32), np.zeros(3, np.float32)
    check(lib().gpp_debug_obs_index(points._h, _ptr(dims), _ptr(geom), None, 0))
    start = np.zeros(int(dims[0]) * int(dims[1]) + 1, np.int32)
    check(lib().gpp_debug_obs_index(points._h, _ptr(dims), _ptr(geom), _ptr(start), start.size))
    return {"nbx": int(dims[0]), "nby": int(dims[1]), "amin": geom[0], "bmin": geom[1], "inv_s": geom[2], "bin_start": start,
            "device_built": bool(dims[2])}


# ---- nearest (src/api/nearest.cpp:124-144) ----------------------------------------------------------
def _interpolate_levels(entry, igrid, opoints, values, rank_message, pad_empty):
    """The body nearest and bilinear share: values on igrid, with or without a leading time dimension -> the same on opoints.
    pad_empty: an empty host array of too few dimensions counts as one of the right number ([] on a Grid is (0, 0))."""
    nd = 2 if isinstance(igrid, Grid) else 1
    f64 = _wants_f64(values)
    values = _m.field(values, f64=f64)
    if pad_empty and not _is_dev(values) and values.size == 0 and values.ndim < nd:
        values = values.reshape((0,) * nd)
    shp = _shape(values)
    if len(shp) not in (nd, nd + 1):
        raise RuntimeError(rank_message)
    levels = len(shp) == nd + 1
    if nd == 2:    # src/api/util.cpp:427-432: no rows (2-D) / no time levels or no rows (3-D) passes the size check
        empty = shp[0] == 0 or (levels and shp[1] == 0)
    else:          # util.cpp:433-438: a vec2 with no time levels passes, a vec must match
        empty = levels and shp[0] == 0
    if not empty and tuple(shp[-nd:]) != _out_shape(igrid):
        raise ValueError("Grid size is not the same as values" if nd == 2 else "Points size is not the same as values")
    nt = shp[0] if levels else 1
    oshape = ((nt,) if levels else ()) + _out_shape(opoints)
    if int(np.prod(oshape)) == 0:
        return _empty_like_field(oshape, values)
    if igrid._n and empty:
        raise ValueError("Grid size is not the same as values")   # nothing to read from (the reference would index past the end)
    return _m.run(entry, igrid._h, opoints._h, _ptr(values), nt, out_shape=oshape, like=values, mem=_m.flags(f64, values))


def nearest(igrid, opoints, values):
    """All eight overloads of src/api/nearest.cpp: Grid|Points -> Grid|Points, with or without a leading time dimension."""
    nd = 2 if isinstance(igrid, Grid) else 1
    return _interpolate_levels(lib().gpp_nearest_levels, igrid, opoints, values, "values must have %d or %d dimensions" % (nd, nd + 1), True)


# ---- count / gridding (include/gridpp.h:938-1010, src/api/count.cpp, src/api/gridding.cpp) -------------
def count(ipoints, opoints, radius):
    """Number of points of `ipoints` (Grid or Points) within `radius` of every location of `opoints` (count.cpp:6-66)."""
    out = np.empty(_out_shape(opoints), np.float32)
    if out.size:
        check(lib().gpp_count(ipoints._h, opoints._h, float(radius), _ptr(out), _capi.MEM_HOST))
    return out


def distance(ipoints, opoints, num):
    """Largest distance from every location of `opoints` to its `num` nearest points of `ipoints` (distance.cpp:6-120)."""
    if ipoints.get_coordinate_type() != opoints.get_coordinate_type():
        raise ValueError("Incompatible coordinate types")
    out = np.empty(_out_shape(opoints), np.float32)
    if out.size:
        check(lib().gpp_distance(ipoints._h, opoints._h, int(num), 0 if isinstance(opoints, Grid) else 1, _ptr(out), _capi.MEM_HOST))
    return out


def staticcorr_points(points, knots, structure, max_points):
    """(L, K) static correlations between a set of points and a set of knots (src/api/corr_points.cpp:26-131)."""
    if max_points < 0:
        raise ValueError("max_points must be >= 0")
    if points.get_coordinate_type() != knots.get_coordinate_type():
        raise ValueError("Both background grid and observations points must be of same coordinate type (lat/lon or x/y)")
    out = _host_empty((points.size(), knots.size()))
    if out.size:
        check(lib().gpp_staticcorr_points(points._h, knots._h, _structure(structure), int(max_points), _ptr(out), _capi.MEM_HOST))
    return out


def _point_values(ipoints, values):
    values = _m.field(values, 1, "values", dev_message="values must have 1 dimension")
    if _shape(values)[0] != ipoints.size():
        raise ValueError("Points size is not the same as values")
    return values


def gridding(grid, points, values, radius, min_num, statistic):
    """gridding.cpp:6-63; `grid` may be a Grid or a Points (output shaped accordingly)."""
    values = _point_values(points, values)
    if not is_valid(radius) or radius < 0:
        raise ValueError("radius must be >= 0")
    if min_num < 0:
        raise ValueError("min_num must be >= 0")
    if int(np.prod(_out_shape(grid))) == 0:
        return _empty_like_field(_out_shape(grid), values)
    return _m.run(lib().gpp_gridding, grid._h, points._h, _ptr(values), float(radius), int(min_num), int(statistic),
                  out_shape=_out_shape(grid), like=values, mem=_m.flags(False, values))


def gridding_nearest(grid, points, values, min_num, statistic):
    """gridding.cpp:65-131"""
    values = _point_values(points, values)
    if min_num < 0:
        raise ValueError("min_num must be >= 0")
    if int(np.prod(_out_shape(grid))) == 0 and not points.size():
        return _empty_like_field(_out_shape(grid), values)
    return _m.run(lib().gpp_gridding_nearest, grid._h, points._h, _ptr(values), int(min_num), int(statistic),
                  out_shape=_out_shape(grid), like=values, mem=_m.flags(False, values))


# ---- fill / doping / neighbourhood_search / calc_gradient -----------------------------------------------
MinMax, LinearRegression = 0, 10   # include/gridpp.h:126-129


def _grid_field(igrid, values, what="values"):
    values = _m.field(values, 2, what)
    shp = _shape(values)
    if shp[0] != 0 and tuple(shp) != tuple(igrid.size()):       # src/api/util.cpp:427-429
        raise ValueError("Grid size is not the same as " + what)
    return values


def fill(igrid, input, points, radii, value, outside):
    """src/api/fill.cpp:6-41"""
    input = _grid_field(igrid, input)
    radii = np.ascontiguousarray(np.asarray(radii, np.float32).ravel())
    if radii.size != points.size():
        raise ValueError("Points size is not the same as radii size")
    if int(np.prod(_shape(input))) == 0:
        return _empty_like_field(_shape(input), input)
    return _m.run(lib().gpp_fill, igrid._h, _ptr(input), points._h, _ptr(radii), float(value), int(bool(outside)),
                  out_shape=_shape(input), like=input, mem=_m.flags(False, input))


def fill_missing(values):
    """src/api/fill.cpp:43-134"""
    f64 = _wants_f64(values)
    values = _m.field(values, 2, "values", f64)
    ny, nx = _shape(values)
    if ny * nx == 0:
        return _empty_like_field((ny, nx), values)
    return _m.run(lib().gpp_fill_missing, _ptr(values), ny, nx, out_shape=(ny, nx), like=values, mem=_m.flags(f64, values))


def _doping(igrid, background, points, observations, halfwidth, radii, max_elev_diff):
    background = _grid_field(igrid, background, "observations")
    observations = _m.field(observations, 1, "observations")
    if _shape(observations)[0] != points.size():
        raise ValueError("Points size is not the same as observations size")
    per = halfwidth if halfwidth is not None else radii
    if per.size != points.size():
        raise ValueError("Points size is not the same as %s size" % ("halfwidth" if halfwidth is not None else "radii"))
    if int(np.prod(_shape(background))) == 0:
        return _empty_like_field(_shape(background), background)
    return _m.run(lib().gpp_doping, igrid._h, _ptr(background), points._h, _ptr(observations), _ptr(halfwidth), _ptr(radii),
                  float(max_elev_diff), out_shape=_shape(background), like=background, mem=_m.flags(False, background, observations))


def doping_square(igrid, background, points, observations, halfwidth, max_elev_diff=MV):
    """src/api/doping.cpp:5-48"""
    return _doping(igrid, background, points, observations, np.ascontiguousarray(np.asarray(halfwidth, np.int32).ravel()), None, max_elev_diff)


def doping_circle(igrid, background, points, observations, radii, max_elev_diff=MV):
    """src/api/doping.cpp:50-93"""
    return _doping(igrid, background, points, observations, None, np.ascontiguousarray(np.asarray(radii, np.float32).ravel()), max_elev_diff)


def neighbourhood_search(array, search_array, halfwidth, search_target_min, search_target_max, search_delta, apply_array=None):
    """src/api/neighbourhood_search.cpp:7-113"""
    f64 = _wants_f64(array, search_array)
    array, search_array = _m.field(array, 2, "array", f64), _m.field(search_array, 2, "search_array", f64)
    if _shape(array) != _shape(search_array):
        raise ValueError("search_array must either be the same size as array")
    if search_target_min > search_target_max:
        raise ValueError("Search_target_min must be smaller than search_target_max")
    if halfwidth < 0:
        raise ValueError("halfwidth must be positive")
    ap = None
    if apply_array is not None and (apply_array.numel() if _is_dev(apply_array) else np.size(apply_array)) > 0:
        ap = _m.field(apply_array, dtype=np.int32)
        # (the reference indexes apply_array[y][x] for every cell whatever its size; anything but a full-size mask reads out of bounds there)
        if tuple(ap.shape) != _shape(array):
            raise ValueError("apply_array must either be empty or same size as array")
    ny, nx = _shape(array)
    if ny * nx == 0:
        return _empty_like_field((ny, nx), array)
    return _m.run(lib().gpp_neighbourhood_search, _ptr(array), _ptr(search_array), ny, nx, int(halfwidth), float(search_target_min),
                  float(search_target_max), float(search_delta), _ptr(ap), out_shape=(ny, nx), like=array,
                  mem=_m.flags(f64, array, search_array, ap))


def calc_gradient(base, values, gradient_type, halfwidth, num_min=2, min_range=MV, default_gradient=0):
    """src/api/calc_gradient.cpp:7-126"""
    f64 = _wants_f64(base, values)
    base, values = _m.field(base, 2, "base", f64), _m.field(values, 2, "values", f64)
    if halfwidth <= 0:
        raise ValueError("Halwidth cannot be <= 0; must be positive integer")
    if is_valid(min_range) and min_range < 0:
        raise ValueError("min_range must be >= 0")
    if num_min < 0:
        raise ValueError("num_min must be >= 0")
    if _shape(base)[0] == 0:
        raise ValueError("base input has no size")
    if _shape(base) != _shape(values):
        raise ValueError("base is not the same size as values")
    ny, nx = _shape(base)
    return _m.run(lib().gpp_calc_gradient, _ptr(base), _ptr(values), ny, nx, int(gradient_type), int(halfwidth), int(num_min),
                  float(min_range), float(default_gradient), out_shape=(ny, nx), like=base, mem=_m.flags(f64, base, values))


# ---- bilinear (include/gridpp.h:902-930, src/api/bilinear.cpp:26-135) ---------------------------------
def bilinear(igrid, opoints, values):
    """values (Y, X) -> output shaped like opoints; values (T, Y, X) -> (T,) + that shape."""
    if not isinstance(igrid, Grid):
        raise TypeError("bilinear: the input must be a Grid")
    return _interpolate_levels(lib().gpp_bilinear, igrid, opoints, values, "bilinear: values must be 2-D or 3-D", False)


# ---- downscaling, simple_gradient, full_gradient (include/gridpp.h:132-135,844-871,1017-1098) ---------------------------
Nearest, Bilinear = 0, 1   # include/gridpp.h:132-135


def _downscale_sets(name, igrid, output):
    if not isinstance(igrid, Grid):
        raise TypeError("%s: the input must be a Grid" % name)
    if not isinstance(output, (Grid, Points)):
        raise TypeError("%s: the output must be a Grid or Points" % name)


def _downscale_setup(name, igrid, output, ivalues, fields=()):
    """Checks shared by the downscalers -> (values, other fields, ndim, output shape, empty, f64).  Fields are float32 arrays (float64
    where f64) or float32 device tensors; None stays None."""
    _downscale_sets(name, igrid, output)
    return _downscale_fields(name, _out_shape(output), ivalues, fields)


def _downscale_fields(name, out_shape, ivalues, fields=()):
    """_downscale_setup once the two sets are known to be a Grid and a Grid or Points; out_shape: the shape of a field on the output"""
    f64 = _wants_f64(ivalues, *fields)
    values = _m.field(ivalues, f64=f64)
    shp = _shape(values)
    if len(shp) not in (2, 3):
        raise RuntimeError("%s: values must be 2-D or 3-D" % name)
    # src/api/util.cpp:427-432: no rows (2-D) / no time levels or no rows (3-D) passes the size check
    empty = shp[0] == 0 or (len(shp) == 3 and shp[1] == 0)
    lead = (shp[0],) if len(shp) == 3 else ()
    return values, [_m.field(a, f64=f64) for a in fields], len(shp), lead + out_shape, empty, f64


def _downscaler(downscaler):
    if downscaler not in (Nearest, Bilinear):   # src/api/downscaling.cpp:16-17
        raise ValueError("Invalid downscaler")
    return int(downscaler)


def downscaling(igrid, output, ivalues, downscaler):
    """src/api/downscaling.cpp:7-61: `nearest` or `bilinear` from a Grid to a Grid or Points, 2-D or 3-D (T, Y, X) values."""
    values, _, _, _, empty, _ = _downscale_setup("downscaling", igrid, output, ivalues)
    if not empty and _shape(values)[-2:] != tuple(igrid.size()):
        raise ValueError("Grid size is not the same as values")
    if _downscaler(downscaler) == Nearest:
        return nearest(igrid, output, values)
    return bilinear(igrid, output, values)


def _gradient_call(entry, igrid, output, values, fields, oshape, empty, f64, downscaler, *args):
    """runs gpp_simple_gradient / gpp_full_gradient once the overload's checks have passed; fields = the present gradients"""
    downscaler = _downscaler(downscaler)
    return _gradient_run(entry, (igrid._h, output._h), igrid._n, values, fields, oshape, empty, f64, *args, downscaler)


def _gradient_run(entry, handles, n_in, values, fields, oshape, empty, f64, *args):
    """entry(*handles, values, nt, *args, out, mem); n_in: the number of points of the input grid"""
    _mem(values, *fields)   # (mixed memory is refused whatever the shapes)
    if int(np.prod(oshape)) == 0:
        return _empty_like_field(oshape, values)
    if n_in and empty:
        raise ValueError("Grid size is not the same as values")   # nothing to read from (the reference would index past the end)
    nt = oshape[0] if len(_shape(values)) == 3 else 1
    return _m.run(entry, *handles, _ptr(values), nt, *args, out_shape=oshape, like=values, mem=_m.flags(f64, values, *fields))


def simple_gradient(igrid, output, ivalues, elev_gradient, downscaler=Nearest):
    """src/api/simple_gradient.cpp: d(values) + (output elevation - d(grid elevation)) * elev_gradient, d = the downscaler.
    No validity test: a missing elevation or gradient gives NaN."""
    values, _, _, oshape, empty, f64 = _downscale_setup("simple_gradient", igrid, output, ivalues)
    if not empty and _shape(values)[-2:] != tuple(igrid.size()):
        raise ValueError("Grid size is not the same as values")
    return _gradient_call(lib().gpp_simple_gradient, igrid, output, values, (), oshape, empty, f64, downscaler, float(elev_gradient))


_NO_LAF = object()


def full_gradient(igrid, output, ivalues, elev_gradient, laf_gradient=_NO_LAF, downscaler=Nearest):
    """src/api/gradient.cpp:5-274: d(values) + (laf_corr + elev_corr), elev_corr = d(elev_gradient) * (output elevation - d(grid
    elevation)) where both elevations are valid (else 0), laf_corr likewise.  A gradient with no elements leaves its term out.
    Gradients have the shape of the values; only the Grid -> Grid 2-D overload may leave out laf_gradient (include/gridpp.h:1065)."""
    _downscale_sets("full_gradient", igrid, output)
    values, egrad, lgrad, oshape, empty, f64 = _full_gradient_fields(tuple(igrid.size()), _out_shape(output), isinstance(output, Grid),
                                                                     ivalues, elev_gradient, laf_gradient)
    return _gradient_call(lib().gpp_full_gradient, igrid, output, values, [g for g in (egrad, lgrad) if g is not None], oshape, empty,
                          f64, downscaler, _ptr(egrad), _ptr(lgrad))


def _full_gradient_fields(ishape, out_shape, out_is_grid, ivalues, elev_gradient, laf_gradient):
    """The overload rules and size checks of full_gradient -> (values, egrad, lgrad, output shape, empty, f64); an absent gradient is None"""
    values, (egrad, lgrad), nd, oshape, empty, f64 = _downscale_fields(
        "full_gradient", out_shape, ivalues, (elev_gradient, None if laf_gradient is _NO_LAF else laf_gradient))
    grid_vec2 = out_is_grid and nd == 2
    if laf_gradient is _NO_LAF:
        if not grid_vec2:
            raise TypeError("full_gradient: laf_gradient is required unless both grids are 2-D fields (include/gridpp.h:1065-1098)")
        lgrad = np.zeros((0, 0), np.float32)
    if grid_vec2:   # gradient.cpp:10-11
        if _shape(values) != ishape:
            raise ValueError("Values is the wrong size")
    elif not empty and _shape(values)[-2:] != ishape:
        raise ValueError("Grid size is not the same as values")   # downscaling.cpp:8-9
    present = []
    # gradient.cpp:13-20 (checked in this order); the other overloads only assert it and would read past the end
    for g, what in ((lgrad, "Laf gradient is the wrong size"), (egrad, "Elevation gradient is the wrong size")):
        n = g.numel() if _is_dev(g) else g.size
        if n == 0:
            present.append(None)
        elif _shape(g) != _shape(values):
            raise ValueError(what)
        else:
            present.append(g)
    lgrad, egrad = present
    return values, egrad, lgrad, oshape, empty, f64


# ---- the reusable downscaling plan (include/gridpp_hip.h: gpp_downscale_plan_*; no counterpart in the reference) -------------------
class DownscalingPlan:
    """What downscaling_plan returns: for every output location the nearest grid point and, for Bilinear, its box and weights."""

    def __init__(self, handle, igrid, output, downscaler):
        self._h, self.downscaler = handle, downscaler
        self._ishape, self._n_in = tuple(igrid.size()), igrid._n
        self._oshape, self._out_grid = _out_shape(output), isinstance(output, Grid)
        self._itype, self._otype = igrid.get_coordinate_type(), output.get_coordinate_type()   # (a Bilinear plan may span two)

    def __del__(self):
        try:
            self.release()
        except Exception:   # noqa: BLE001  (interpreter shutdown)
            pass

    def release(self):
        """gpp_downscale_plan_destroy: returns the HBM the plan holds (`nbytes`); the plan cannot be used afterwards."""
        h, self._h = self._h, None
        if h:
            check(lib().gpp_downscale_plan_destroy(h))

    def _handle(self):
        if not self._h:
            raise RuntimeError("the plan was released")
        return self._h

    def apply(self, values):
        """downscaling(igrid, output, values, downscaler), bit for bit: values (Y, X) or (T, Y, X)."""
        h = self._handle()
        values, _, _, oshape, empty, f64 = _downscale_fields("downscaling", self._oshape, values)
        if not empty and _shape(values)[-2:] != self._ishape:
            raise ValueError("Grid size is not the same as values")
        return _gradient_run(lib().gpp_downscale_plan_apply, (h,), self._n_in, values, (), oshape, empty, f64)

    def apply_cube(self, values):
        """An ensemble in gridpp's cube layout, (Y, X, E) -> (oY, oX, E) or (N, E): plane [..., e] is downscaling(igrid, output,
        values[..., e], downscaler), bit for bit.  For Bilinear the four-corner validity test is per member and location."""
        h = self._handle()
        f64 = _wants_f64(values)
        values = _m.field(values, f64=f64)
        shp = _shape(values)
        if len(shp) != 3:
            raise RuntimeError("apply_cube: values must be 3-D (Y, X, E)")
        if shp[:2] != self._ishape:
            raise ValueError("Grid size is not the same as values")
        oshape = self._oshape + (shp[2],)
        if int(np.prod(oshape)) == 0:
            return _empty_like_field(oshape, values)
        return _m.run(lib().gpp_downscale_plan_apply_cube, h, _ptr(values), shp[2], out_shape=oshape, like=values, mem=_m.flags(f64, values))

    def simple_gradient(self, values, elev_gradient):
        """simple_gradient(igrid, output, values, elev_gradient, downscaler), bit for bit."""
        h = self._handle()
        values, _, _, oshape, empty, f64 = _downscale_fields("simple_gradient", self._oshape, values)
        if not empty and _shape(values)[-2:] != self._ishape:
            raise ValueError("Grid size is not the same as values")
        return _gradient_run(lib().gpp_downscale_plan_simple_gradient, (h,), self._n_in, values, (), oshape, empty, f64, float(elev_gradient))

    def full_gradient(self, values, elev_gradient, laf_gradient=_NO_LAF):
        """full_gradient(igrid, output, values, elev_gradient, laf_gradient, downscaler), bit for bit, with its overload rules."""
        h = self._handle()
        values, egrad, lgrad, oshape, empty, f64 = _full_gradient_fields(self._ishape, self._oshape, self._out_grid, values, elev_gradient,
                                                                         laf_gradient)
        return _gradient_run(lib().gpp_downscale_plan_full_gradient, (h,), self._n_in, values, [g for g in (egrad, lgrad) if g is not None],
                             oshape, empty, f64, _ptr(egrad), _ptr(lgrad))

    # ---- gradients on gridpp's cube layout ----
    def _cube(self, name, values, f64):
        """the (Y, X, E) values of a cube method -> (values, output shape)"""
        values = _m.field(values, f64=f64)
        shp = _shape(values)
        if len(shp) != 3:
            raise RuntimeError("%s: values must be 3-D (Y, X, E)" % name)
        if shp[:2] != self._ishape:
            raise ValueError("Grid size is not the same as values")
        return values, self._oshape + (shp[2],)

    def simple_gradient_cube(self, values, elev_gradient):
        """An ensemble in gridpp's cube layout, (Y, X, E) -> (oY, oX, E) or (N, E): plane [..., e] is simple_gradient(igrid, output,
        values[..., e], elev_gradient, downscaler), bit for bit.  elev_gradient is a scalar."""
        h = self._handle()
        f64 = _wants_f64(values)
        values, oshape = self._cube("simple_gradient_cube", values, f64)
        if int(np.prod(oshape)) == 0:
            return _empty_like_field(oshape, values)
        return _m.run(lib().gpp_downscale_plan_simple_gradient_cube, h, _ptr(values), oshape[-1], float(elev_gradient), out_shape=oshape,
                      like=values, mem=_m.flags(f64, values))

    def full_gradient_cube(self, values, elev_gradient, laf_gradient):
        """An ensemble in gridpp's cube layout, (Y, X, E) -> (oY, oX, E) or (N, E): plane [..., e] is full_gradient(igrid, output,
        values[..., e], elev_gradient_e, laf_gradient_e, downscaler), bit for bit.  Each gradient is (Y, X), one field shared by the
        members, or (Y, X, E), a field per member, or empty ([] or None): the term is absent.  The two may take different forms."""
        h = self._handle()
        f64 = _wants_f64(values, elev_gradient, laf_gradient)
        values, oshape = self._cube("full_gradient_cube", values, f64)
        vshape = _shape(values)
        grads = []
        # the laf gradient first, as gradient.cpp:13-20
        for g, what in ((laf_gradient, "Laf gradient is the wrong size"), (elev_gradient, "Elevation gradient is the wrong size")):
            g = _m.field(g, f64=f64)
            if g is None or (g.numel() if _is_dev(g) else g.size) == 0:
                grads.append((None, 1))
            elif _shape(g) == vshape[:2]:
                grads.append((g, 1))
            elif _shape(g) == vshape:
                grads.append((g, vshape[2]))
            else:
                raise ValueError(what)
        (lgrad, lmembers), (egrad, emembers) = grads
        present = [g for g in (egrad, lgrad) if g is not None]
        _mem(values, *present)
        if int(np.prod(oshape)) == 0:
            return _empty_like_field(oshape, values)
        return _m.run(lib().gpp_downscale_plan_full_gradient_cube, h, _ptr(values), vshape[2], _ptr(egrad), emembers, _ptr(lgrad), lmembers,
                      out_shape=oshape, like=values, mem=_m.flags(f64, values, *present))

    # ---- the ensemble downscalers with the plan's nearest grid points: no search ----
    def _ens(self, name, cubes, threshold, comparison_operator):
        h = self._handle()
        if not self._out_grid:
            raise TypeError("%s: the plan's output must be a Grid" % name)
        return (h,) + _ens_checks(name, self._ishape, self._n_in, self._oshape, self._itype == self._otype, cubes, threshold,
                                  comparison_operator)

    def _ens_run(self, entry, h, cubes, ne, threshold, f64, *args):
        if int(np.prod(self._oshape)) == 0:
            return _empty_like_field(self._oshape, threshold)
        return _m.run(entry, h, *[_ptr(c) for c in cubes], int(ne), _ptr(threshold), *args, out_shape=self._oshape, like=threshold,
                      mem=_m.flags(f64, threshold, *cubes))

    def downscale_probability(self, ivalues, threshold, comparison_operator):
        """downscale_probability(igrid, ogrid, ivalues, threshold, comparison_operator), bit for bit, for a plan built to a Grid."""
        h, cubes, threshold, ne, f64 = self._ens("downscale_probability", [ivalues], threshold, comparison_operator)
        return self._ens_run(lib().gpp_downscale_plan_probability, h, cubes, ne, threshold, f64, int(comparison_operator))

    def _mask_threshold(self, name, ivalues_true, ivalues_false, threshold_values, threshold, comparison_operator, statistic, quantile):
        h, cubes, threshold, ne, f64 = self._ens(name, [ivalues_true, ivalues_false, threshold_values], threshold, comparison_operator)
        _mask_statistic_checks(statistic, quantile)
        return self._ens_run(lib().gpp_downscale_plan_mask_threshold, h, cubes, ne, threshold, f64, int(comparison_operator), int(statistic),
                             float(quantile))

    def mask_threshold_downscale_consensus(self, ivalues_true, ivalues_false, threshold_values, threshold, comparison_operator, statistic):
        """mask_threshold_downscale_consensus(igrid, ogrid, ...), bit for bit (RandomChoice: one of the cell's valid masked members)."""
        return self._mask_threshold("mask_threshold_downscale_consensus", ivalues_true, ivalues_false, threshold_values, threshold,
                                    comparison_operator, statistic, 0.0)

    def mask_threshold_downscale_quantile(self, ivalues_true, ivalues_false, threshold_values, threshold, comparison_operator, quantile):
        """mask_threshold_downscale_quantile(igrid, ogrid, ...), bit for bit."""
        return self._mask_threshold("mask_threshold_downscale_quantile", ivalues_true, ivalues_false, threshold_values, threshold,
                                    comparison_operator, Quantile, quantile)

    def _info(self):
        locations, cells, nbytes, distorted = C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_longlong()
        downscaler = C.c_int()
        check(lib().gpp_downscale_plan_info(self._handle(), C.byref(locations), C.byref(cells), C.byref(downscaler), C.byref(nbytes),
                                            C.byref(distorted)))
        return locations.value, cells.value, downscaler.value, nbytes.value, distorted.value

    @property
    def nbytes(self):
        """HBM the plan holds: 4 (Nearest) or 16 (Bilinear) bytes per output location, plus the elevations and lafs of both sets."""
        return self._info()[3]

    @property
    def distorted(self):
        """output locations whose bilinear weights leave [0, 1]: an apply raises there once a field has four valid corners"""
        return self._info()[4]


def downscaling_plan(igrid, output, downscaler=Nearest):
    """Everything of downscaling, simple_gradient and full_gradient that does not depend on a value, computed once: the nearest grid
    point of every output location and, for Bilinear, its box and weights (src/api/grid.cpp:149-229, bilinear.cpp:137-320).

        plan = downscaling_plan(igrid, ogrid, Bilinear)
        out = plan.apply(values)                    # = downscaling(igrid, ogrid, values, Bilinear)
        out = plan.apply_cube(values_yxe)           # an ensemble in gridpp's cube layout, E innermost
        out = plan.full_gradient(values, egrad, lgrad)

    instead of a loop of direct calls over lead times, members or variables on the same pair of grids.  The plan holds 4 (Nearest) or
    16 (Bilinear) bytes of HBM per output location plus copies of both sets' elevations and lafs (`nbytes`) until release() or until
    it is garbage-collected; igrid and output may be dropped first.  A box whose weights leave [0, 1] does not fail the construction
    (`distorted` counts them): the methods raise where the direct calls do."""
    _downscale_sets("downscaling_plan", igrid, output)
    downscaler = _downscaler(downscaler)
    if downscaler == Nearest and igrid.get_coordinate_type() != output.get_coordinate_type():
        raise ValueError("Coordinate types must be the same")
    handle = C.c_void_p()
    check(lib().gpp_downscale_plan_create(igrid._h, output._h, downscaler, C.byref(handle)))
    return DownscalingPlan(handle, igrid, output, downscaler)


# ---- ensemble downscalers and smart (include/gridpp.h:138-143,945-990,1112) ----------------------------------------------
Lt, Leq, Gt, Geq = 0, 10, 20, 30   # include/gridpp.h:138-143


def _ens_setup(name, igrid, ogrid, cubes, threshold, comparison_operator):
    """The checks the ensemble downscalers share (the reference checks none: a wrong shape reads out of bounds there) ->
    (cubes, threshold, ne, f64).  Cubes are (Y, X, E), the threshold (oY, oX)."""
    if not isinstance(igrid, Grid) or not isinstance(ogrid, Grid):
        raise TypeError("%s: igrid and ogrid must be Grids" % name)
    return _ens_checks(name, tuple(igrid.size()), igrid._n, tuple(ogrid.size()), igrid.get_coordinate_type() == ogrid.get_coordinate_type(),
                       cubes, threshold, comparison_operator)


def _ens_checks(name, ishape, n_in, oshape, same_types, cubes, threshold, comparison_operator):
    """_ens_setup once the two grids are known by their shapes (n_in: the cells of the input grid) and coordinate types"""
    f64 = _wants_f64(*cubes)
    cubes = [_m.field(a, 3, "values", f64) for a in cubes]
    threshold = _m.field(threshold, 2, "threshold", f64)
    _mem(threshold, *cubes)
    shp = _shape(cubes[0])
    if any(_shape(c) != shp for c in cubes[1:]):
        raise ValueError("%s: ivalues_true, ivalues_false and threshold_values must have the same shape" % name)
    if n_in and shp[:2] != ishape:
        raise ValueError("Grid size is not the same as values")
    if _shape(threshold) != oshape:
        raise ValueError("Grid size is not the same as threshold")
    if not same_types:
        raise ValueError("Coordinate types must be the same")
    if comparison_operator not in (Lt, Leq, Gt, Geq):
        raise ValueError("Invalid comparison operator")
    return cubes, threshold, shp[2], f64


def _mask_statistic_checks(statistic, quantile):
    if statistic not in (Mean, Min, Median, Max, Quantile, Std, Variance, Sum, Count, RandomChoice):   # src/api/util.cpp:106-108
        raise RuntimeError("Internal error. Cannot compute statistic")
    if statistic == Quantile and (quantile < 0 or quantile > 1):   # util.cpp:112-113
        raise ValueError("calc_quantile: Quantile must be between 0 and 1 inclusive")


def _ens_call(entry, igrid, ogrid, cubes, ne, threshold, f64, *args):
    if ogrid._n == 0:
        return _empty_like_field(_out_shape(ogrid), threshold)
    return _m.run(entry, igrid._h, ogrid._h, *[_ptr(c) for c in cubes], int(ne), _ptr(threshold), *args, out_shape=_out_shape(ogrid),
                  like=threshold, mem=_m.flags(f64, threshold, *cubes))


def downscale_probability(igrid, ogrid, ivalues, threshold, comparison_operator):
    """src/api/downscale_probability.cpp:7-67: the share of the valid members of the nearest input cell with
    member OP threshold[i][j]; NaN where no member is valid.  ivalues is (Y, X, E), threshold (oY, oX)."""
    cubes, threshold, ne, f64 = _ens_setup("downscale_probability", igrid, ogrid, [ivalues], threshold, comparison_operator)
    return _ens_call(lib().gpp_downscale_probability, igrid, ogrid, cubes, ne, threshold, f64, int(comparison_operator))


def _mask_threshold_downscale(name, igrid, ogrid, ivalues_true, ivalues_false, threshold_values, threshold, comparison_operator,
                              statistic, quantile):
    cubes, threshold, ne, f64 = _ens_setup(name, igrid, ogrid, [ivalues_true, ivalues_false, threshold_values], threshold,
                                           comparison_operator)
    _mask_statistic_checks(statistic, quantile)
    return _ens_call(lib().gpp_mask_threshold_downscale, igrid, ogrid, cubes, ne, threshold, f64, int(comparison_operator), int(statistic),
                     float(quantile))


def mask_threshold_downscale_consensus(igrid, ogrid, ivalues_true, ivalues_false, threshold_values, threshold, comparison_operator, statistic):
    """src/api/mask_threshold_downscale_consensus.cpp:12-14,19-82: per output cell, member k comes from ivalues_true where
    threshold_values[I][J][k] OP threshold[i][j], from ivalues_false otherwise (NaN where threshold_values is not valid), at the
    nearest input cell (I, J); the members are reduced with `statistic` (Quantile: quantile 0, as the reference passes it)."""
    return _mask_threshold_downscale("mask_threshold_downscale_consensus", igrid, ogrid, ivalues_true, ivalues_false, threshold_values,
                                     threshold, comparison_operator, statistic, 0.0)


def mask_threshold_downscale_quantile(igrid, ogrid, ivalues_true, ivalues_false, threshold_values, threshold, comparison_operator, quantile):
    """src/api/mask_threshold_downscale_consensus.cpp:15-17: the same masked members reduced with calc_quantile(quantile)."""
    return _mask_threshold_downscale("mask_threshold_downscale_quantile", igrid, ogrid, ivalues_true, ivalues_false, threshold_values,
                                     threshold, comparison_operator, Quantile, quantile)


def smart(igrid, ogrid, ivalues, num, structure):
    """src/api/smart.cpp:12-66: the mean of the `num` input cells most correlated (structure.corr) with the output cell among
    those within the structure's localization distance; rho descending, ties -> lower index of the input grid.  No validity
    test on the values.  NaN where there is no candidate or num <= 0."""
    if not isinstance(igrid, Grid) or not isinstance(ogrid, Grid):
        raise TypeError("smart: igrid and ogrid must be Grids")
    st = _structure(structure)
    f64 = _wants_f64(ivalues)
    values = _m.field(ivalues, 2, "values", f64)
    if igrid._n and _shape(values) != tuple(igrid.size()):
        raise ValueError("Grid size is not the same as values")
    if igrid.get_coordinate_type() != ogrid.get_coordinate_type():
        raise ValueError("Coordinate types must be the same")
    if ogrid._n == 0:
        return _empty_like_field(_out_shape(ogrid), values)
    return _m.run(lib().gpp_smart, igrid._h, ogrid._h, _ptr(values), int(num), st, out_shape=_out_shape(ogrid), like=values,
                  mem=_m.flags(f64, values))


# ---- local_distribution_correction (include/gridpp.h:467-512) ---------------------------------------------------------------
def local_distribution_correction(bgrid, background, points, pobs, pbackground, structure, min_quantile, max_quantile, min_points=0):
    """src/api/local_distribution_correction.cpp:18-203: per grid cell, the valid non-negative (pobs, pbackground) pairs of the
    stations within the structure's localization distance, weighted by rho = corr_background(cell, station), form two
    cumulative-rho curves between min_quantile and max_quantile; the cell's background is mapped from the one to the other.
    pobs and pbackground are both 1-D (S) or both 2-D (T, S).  Cells with an invalid background or fewer than min_points pairs
    keep their background.

    Both curves are sorted by value and, where values tie, by rho ascending.  The reference sorts by value alone with an
    unstable sort: on tied values (zeros of precipitation) its result depends on the order its R-tree returns the stations in;
    on tie-free data the two agree.  Shapes the reference would read out of bounds with are refused."""
    if not isinstance(bgrid, Grid) or not isinstance(points, Points):
        raise TypeError("local_distribution_correction: bgrid must be a Grid, points a Points")
    st = _structure(structure)
    fields = (background, pobs, pbackground)
    dev = all(_is_dev(a) for a in fields)
    f64 = not dev and all(isinstance(a, np.ndarray) and a.dtype == np.float64 for a in fields)
    nd = _ndim(pobs)
    if nd not in (1, 2) or _ndim(pbackground) != nd:
        raise ValueError("pobs and pbackground must both be 1-D (points) or both 2-D (times, points)")
    background = _m.field(background, 2, "background", f64)
    pobs, pbackground = _m.field(pobs, nd, "pobs", f64), _m.field(pbackground, nd, "pbackground", f64)
    _mem(background, pobs, pbackground)   # (mixed memory is refused before the shapes are compared)
    if nd == 1:
        pobs, pbackground = pobs.reshape(1, -1), pbackground.reshape(1, -1)   # :27-31
    so, sb = _shape(pobs), _shape(pbackground)
    if so[0] != sb[0]:   # :50-54
        raise ValueError("pobs (%d,%d) is not the same size as pbackground (%d,%d)" % (so + sb))
    if so != sb:
        raise ValueError("pobs (%d,%d) is not the same shape as pbackground (%d,%d)" % (so + sb))
    if _shape(background) != tuple(bgrid.size()):
        raise ValueError("input field %s is not the same size as the grid %s" % (_shape(background), tuple(bgrid.size())))
    if so[1] != points.size():
        raise ValueError("pobs (%d) and points (%d) size mismatch" % (so[1], points.size()))
    if bgrid.get_coordinate_type() != points.get_coordinate_type():
        raise ValueError("Both background grid and observations points must be of same coordinate type (lat/lon or x/y)")
    min_quantile, max_quantile = float(min_quantile), float(max_quantile)
    if not (np.isfinite(min_quantile) and np.isfinite(max_quantile) and 0 <= min_quantile <= max_quantile <= 1):
        raise ValueError("min_quantile and max_quantile must be finite with 0 <= min_quantile <= max_quantile <= 1")
    if bgrid._n == 0:
        return _empty_like_field(_out_shape(bgrid), background)
    return _m.run(lib().gpp_local_distribution_correction, bgrid._h, _ptr(background), points._h, _ptr(pobs), _ptr(pbackground), so[0], st,
                  min_quantile, max_quantile, int(min_points), out_shape=_out_shape(bgrid), like=background,
                  mem=_m.flags(f64, background, pobs, pbackground))


# ---- calibration by a curve (include/gridpp.h:79-85,731-789,1549-1557) -----------------------------------------------------
OneToOne, MeanSlope, NearestSlope, Zero, Unchanged = 0, 10, 20, 30, 40   # include/gridpp.h:79-85
_POLICIES = (OneToOne, MeanSlope, NearestSlope, Zero, Unchanged)


def _host_curve(a):
    """A curve argument of the host-side forms -> C-contiguous float32 numpy array of any ndim."""
    if hasattr(a, "detach") and hasattr(a, "cpu"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def _curve_pair(curve_ref, curve_fcst):
    """The two 1-D curves with the checks of src/api/curve.cpp:7-10."""
    cr, cf = _host_curve(curve_ref), _host_curve(curve_fcst)
    if cr.ndim != 1 or cf.ndim != 1:
        raise ValueError("curve_ref and curve_fcst must be 1-D arrays (one curve) or 3-D arrays (one curve per cell)")
    if cr.size != cf.size:
        raise ValueError("curve_ref and curve_fcst must be the same size")
    if cr.size == 0:
        raise ValueError("curve_ref and curve_fcst cannot have size 0")
    return cr, cf


def _values_call(entry, values, *args):
    """An element-wise array form: values (1-D or 2-D, host or torch CUDA) -> an array of the same shape."""
    nd = _ndim(values)
    if nd not in (1, 2):
        raise RuntimeError("input must be a scalar or have 1 or 2 dimensions, got %d" % nd)
    f64 = _wants_f64(values)
    v = _m.field(values, f64=f64)
    shp = _shape(v)
    n = int(np.prod(shp))
    if n == 0:
        return np.zeros(shp, np.float32)
    return _m.run(entry, _ptr(v), n, *args, out_shape=shp, like=v, mem=_m.flags(f64, v))


def apply_curve(fcst, curve_ref, curve_fcst, policy_below, policy_above):
    """src/api/curve.cpp:6-133, all four overloads: a scalar, a 1-D or a 2-D field through one curve (1-D curves), or a 2-D
    field through one curve per cell (curves (Y, X, C)).  Inside [curve_fcst[0], curve_fcst[-1]] the result is
    interpolate(fcst, curve_fcst, curve_ref); outside, nearest_ref + slope * (fcst - nearest_fcst) with the slope of the
    policy (Unchanged: the input).  Any curve works, sorted or not, with the reference's linear-scan rules.  The array forms
    refuse an unknown policy whatever the data; the scalar form, like the reference, only where the input extrapolates with it."""
    nd_ref, nd_fcst = _ndim(curve_ref), _ndim(curve_fcst)
    if nd_ref == 3 or nd_fcst == 3:
        return _apply_curve_field(fcst, curve_ref, curve_fcst, policy_below, policy_above)
    cr, cf = _curve_pair(curve_ref, curve_fcst)
    if _ndim(fcst) == 0:
        out = C.c_float(np.nan)
        check(lib().gpp_apply_curve_scalar(float(fcst), _ptr(cr), cr.size, _ptr(cf), cf.size, int(policy_below), int(policy_above), C.byref(out)))
        return out.value
    if policy_below not in _POLICIES or policy_above not in _POLICIES:
        raise ValueError("Unknown extrapolation policy")
    return _values_call(lib().gpp_apply_curve, fcst, _ptr(cr), cr.size, _ptr(cf), cf.size, int(policy_below), int(policy_above))


def _apply_curve_field(fcst, curve_ref, curve_fcst, policy_below, policy_above):
    if _ndim(curve_ref) != 3 or _ndim(curve_fcst) != 3:
        raise ValueError("curve_ref and curve_fcst dimension sizes mismatch")
    if _ndim(fcst) != 2:
        raise ValueError("Fcst and curve_ref dimension sizes mismatch")
    f64 = _wants_f64(fcst, curve_ref, curve_fcst)
    v, cr, cf = _m.field(fcst, 2, "fcst", f64), _m.field(curve_ref, 3, "curve_ref", f64), _m.field(curve_fcst, 3, "curve_fcst", f64)
    _mem(v, cr, cf)   # (mixed memory is refused before the shapes are compared)
    if _shape(cr) != _shape(cf):   # curve.cpp:111-116
        raise ValueError("curve_ref and curve_fcst dimension sizes mismatch")
    if _shape(v) != _shape(cr)[:2]:
        raise ValueError("Fcst and curve_ref dimension sizes mismatch")
    ny, nx, nc = _shape(cr)
    if ny * nx > 0 and nc == 0:
        raise ValueError("curve_ref and curve_fcst cannot have size 0")
    if policy_below not in _POLICIES or policy_above not in _POLICIES:
        raise ValueError("Unknown extrapolation policy")
    if ny * nx == 0:
        return np.zeros((ny, nx), np.float32)
    return _m.run(lib().gpp_apply_curve_field, _ptr(v), _ptr(cr), _ptr(cf), ny, nx, nc, nc, int(policy_below), int(policy_above),
                  out_shape=(ny, nx), like=v, mem=_m.flags(f64, v, cr, cf))


def interpolate(x, iX, iY):
    """src/api/util.cpp:377-426, scalar and vector forms: the curve (iX, iY) at x with the reference's linear-scan index rules
    (invalid entries are skipped, duplicates of iX follow util.cpp:398-407); the end value outside [iX[0], iX[-1]], NaN for a
    NaN x or an empty curve.  Where iX[0] is not valid the reference can reach an undefined index; this returns NaN there and
    reads nothing out of bounds (outside the pinned behaviour)."""
    ix, iy = _host_curve(iX), _host_curve(iY)
    if ix.ndim != 1 or iy.ndim != 1:
        raise RuntimeError("iX and iY must have 1 dimension")
    if _ndim(x) == 0:
        out = C.c_float(np.nan)
        check(lib().gpp_interpolate_scalar(float(x), _ptr(ix), ix.size, _ptr(iy), iy.size, C.byref(out)))
        return out.value
    if ix.size != iy.size:
        raise ValueError("Dimension mismatch. Cannot interpolate.")
    if _ndim(x) != 1:
        raise RuntimeError("x must be a scalar or have 1 dimension")
    return _values_call(lib().gpp_interpolate, x, _ptr(ix), ix.size, _ptr(iy), iy.size)


def quantile_mapping_curve(ref, fcst, quantiles=()):
    """src/api/quantile_mapping.cpp:5-46 -> (curve_ref, curve_fcst): both inputs sorted; sizes 0 and 1 are returned as given.
    With quantiles (each in [0, 1], else ValueError) entry i is element int(float32(q) * float32(S - 1)) of the inputs AS GIVEN,
    not of the sorted copies: the reference indexes `ref` / `fcst` there (:41-42) and this reproduces it.  NaN inputs (no
    defined order in the reference's std::sort) sort last."""
    r, f = _host_curve(ref).ravel(), _host_curve(fcst).ravel()
    q = _host_curve(quantiles).ravel()
    n = max(r.size, f.size, q.size, 1)
    out_ref, out_fcst = np.empty(n, np.float32), np.empty(n, np.float32)
    count = C.c_int(0)
    check(lib().gpp_quantile_mapping_curve(_ptr(r), r.size, _ptr(f), f.size, _ptr(q), q.size, _ptr(out_ref), _ptr(out_fcst), C.byref(count)))
    return out_ref[:count.value].copy(), out_fcst[:count.value].copy()


def monotonize_curve(curve_ref, curve_fcst):
    """src/api/curve.cpp:134-250 -> (curve_ref, curve_fcst): pairs with a missing member are dropped, then every stretch where
    curve_fcst does not increase by more than 0.1 is removed.  Two empty arrays where no pair is valid (the reference reads
    an empty vector there)."""
    cr, cf = _host_curve(curve_ref).ravel(), _host_curve(curve_fcst).ravel()
    n = max(cr.size, cf.size, 1)
    out_ref, out_fcst = np.empty(n, np.float32), np.empty(n, np.float32)
    count = C.c_int(0)
    check(lib().gpp_monotonize_curve(_ptr(cr), cr.size, _ptr(cf), cf.size, _ptr(out_ref), _ptr(out_fcst), C.byref(count)))
    return out_ref[:count.value].copy(), out_fcst[:count.value].copy()


def point_in_rectangle(A, B, C_, D, m):   # src/api/util.cpp:571-582
    corners = (C.c_float * 8)(A.lat, A.lon, B.lat, B.lon, C_.lat, C_.lon, D.lat, D.lon)
    inside = C.c_int(0)
    check(lib().gpp_point_in_rectangle(corners, float(m.lat), float(m.lon), C.byref(inside)))
    return bool(inside.value)


# ---- neighbourhood filters (include/gridpp.h:588-716, src/api/neighbourhood.cpp) ---------------------
def _field23(a, name="input", keep_f64=False):
    """2-D or 3-D field -> (array, ny, nx, ne, is3d, f64); [[]] -> empty.  keep_f64: a large float64 array stays float64 (f64 is
    then true, for the caller's flags)."""
    f64 = keep_f64 and _wants_f64(a)
    arr = _m.field(a, f64=f64)
    nd = len(_shape(arr))
    if nd not in (2, 3):
        if getattr(arr, "size", 1) == 0:
            return arr, 0, 0, 0, 0, f64
        raise RuntimeError("%s must have 2 or 3 dimensions" % name)
    shp = tuple(arr.shape)
    ny, nx = shp[0], shp[1]
    ne = shp[2] if nd == 3 else 1
    return arr, ny, nx, ne, int(nd == 3), f64


def neighbourhood(input, halfwidth, statistic):
    """gridpp::neighbourhood for 2-D and 3-D (Y, X, E) input (src/api/neighbourhood.cpp:12-242)."""
    arr, ny, nx, ne, is3d, f64 = _field23(input, keep_f64=True)
    if halfwidth < 0:
        raise ValueError("Half width must be > 0")
    if statistic == Quantile:
        raise ValueError("Use neighbourhood_quantile for computing neighbourhood quantiles")
    if ny * nx * ne == 0:
        return np.zeros((0, 0), np.float32)
    return _m.run(lib().gpp_neighbourhood, _ptr(arr), ny, nx, ne, is3d, int(halfwidth), int(statistic), out_shape=(ny, nx), like=arr,
                  mem=_m.flags(f64, arr))


def _brute_force(input, halfwidth, statistic, quantile):
    """the body neighbourhood_brute_force and neighbourhood_quantile share"""
    arr, ny, nx, ne, is3d, _ = _field23(input)
    if halfwidth < 0:
        raise ValueError("Half width must be > 0")
    if ny * nx * ne == 0:
        return np.zeros((0, 0), np.float32)
    return _m.run(lib().gpp_neighbourhood_brute_force, _ptr(arr), ny, nx, ne, int(halfwidth), int(statistic), float(quantile), out_shape=(ny, nx),
                  like=arr, mem=_m.flags(False, arr))


def neighbourhood_brute_force(input, halfwidth, statistic):
    return _brute_force(input, halfwidth, statistic, 0.0)


def neighbourhood_quantile(input, quantile, halfwidth):
    """Exact neighbourhood quantile (src/api/neighbourhood.cpp:534-539)."""
    return _brute_force(input, halfwidth, Quantile, quantile)


def neighbourhood_quantile_fast(input, quantile, halfwidth, thresholds):
    """All four overloads of gridpp::neighbourhood_quantile_fast (src/api/neighbourhood.cpp:296-527)."""
    arr, ny, nx, ne, is3d, f64 = _field23(input, keep_f64=True)
    if halfwidth < 0:
        raise ValueError("Half width must be > 0")
    if ny * nx * ne == 0:
        return np.zeros((0, 0), np.float32)
    if np.ndim(quantile) == 0 and not _is_dev(quantile):
        q = np.array([quantile], np.float32)
    else:
        q = _m.field(quantile, 2, "quantile")
        if _shape(q) not in ((1, 1), (ny, nx)):
            raise ValueError("Quantile must be the same size as input, or size (1, 1)")
    thr = _m.field(thresholds, 1, "thresholds")
    nq = int(np.prod(_shape(q)))
    q_host = False
    if _is_dev(arr):
        import torch
        if not _is_dev(q) and nq == 1:
            q_host = True        # (a scalar beside a device-resident field stays on the host: GPP_Q_HOST)
            q = np.ascontiguousarray(q, np.float32)
        else:
            q = q if _is_dev(q) else torch.from_numpy(np.asarray(q)).to(arr.device)
        thr = thr if _is_dev(thr) else torch.from_numpy(np.asarray(thr)).to(arr.device)
    return _m.run(lib().gpp_neighbourhood_quantile_fast, _ptr(arr), ny, nx, ne, is3d, _ptr(q), nq, int(halfwidth), _ptr(thr),
                  int(_shape(thr)[0]), out_shape=(ny, nx), like=arr, mem=_m.flags(f64, arr) | (_capi.Q_HOST if q_host else 0))


def _dev_thresholds(thr, arr):
    """thresholds beside a device-resident field go to its device"""
    if _is_dev(arr) and not _is_dev(thr):
        import torch
        return torch.from_numpy(np.asarray(thr)).to(arr.device)
    return thr


def neighbourhood_quantiles_fast(input, quantiles, halfwidth, thresholds):
    """Many levels of neighbourhood_quantile_fast from one call (no counterpart in the reference): (Y, X, Q) float32,
    plane [..., j] holding exactly the bits neighbourhood_quantile_fast(input, quantiles[j], halfwidth, thresholds) returns.  The
    member pass over the cube and the window sums do not depend on the level: they run once for all Q.

    input: (Y, X) or (Y, X, E), numpy or a torch CUDA tensor (then the result is one), as for neighbourhood_quantile_fast.
    quantiles: a 1-D sequence of scalar levels in host memory, in any order, repeats allowed; a level outside [0, 1] raises
    ValueError before any device work, a NaN level gives a NaN plane.  Per-cell level fields stay with the single-level function.
    No thresholds: NaN everywhere.  See neighbourhood_cdf for the curve the levels are read from."""
    arr, ny, nx, ne, is3d, f64 = _field23(input, keep_f64=True)
    if halfwidth < 0:
        raise ValueError("Half width must be > 0")
    if ny * nx * ne == 0:
        return np.zeros((0, 0, 0), np.float32)
    q = _m.field(quantiles, 1, "quantiles") if not _is_dev(quantiles) else _m.field(quantiles.cpu().numpy(), 1, "quantiles")
    with np.errstate(invalid="ignore"):
        if np.any((q < 0) | (q > 1)):    # (NaN passes)
            raise ValueError("All quantiles must be >= 0 and <= 1")
    thr = _dev_thresholds(_m.field(thresholds, 1, "thresholds"), arr)
    nq = int(q.size)
    if nq == 0:
        return _m._empty_like_field((ny, nx, 0), arr)
    return _m.run(lib().gpp_neighbourhood_quantiles_fast, _ptr(arr), ny, nx, ne, is3d, _ptr(q), nq, int(halfwidth), _ptr(thr),
                  int(_shape(thr)[0]), out_shape=(ny, nx, nq), like=arr, mem=_m.flags(f64, arr, thr))


def neighbourhood_cdf(input, thresholds, halfwidth):
    """The curve neighbourhood_quantile_fast interpolates in (the reference computes it and throws it away,
    src/api/neighbourhood.cpp:490-509): (Y, X, T) float32, plane [..., t] = P(member <= thresholds[t]) over the window of
    halfwidth and the members -- the per-cell fraction float(sum) / count, its neighbourhood Mean, the E-fold float32 sum / E, clamped
    to [0, 1].  The planes follow the thresholds as given (unsorted, duplicated, non-finite ones included); a value is NaN where
    the window holds no valid cell.  The exceedance probability P(member > threshold) is 1 - cdf.

    interpolate(q, cdf[y, x, :], thresholds) in float32 (with the two special cases of neighbourhood.cpp:514-517) gives the bits
    of neighbourhood_quantile_fast(input, q, halfwidth, thresholds) wherever the column holds no NaN."""
    arr, ny, nx, ne, is3d, f64 = _field23(input, keep_f64=True)
    if halfwidth < 0:
        raise ValueError("Half width must be > 0")
    if ny * nx * ne == 0:
        return np.zeros((0, 0, 0), np.float32)
    thr = _dev_thresholds(_m.field(thresholds, 1, "thresholds"), arr)
    nt = int(_shape(thr)[0])
    if nt == 0:
        return _m._empty_like_field((ny, nx, 0), arr)
    return _m.run(lib().gpp_neighbourhood_cdf, _ptr(arr), ny, nx, ne, is3d, int(halfwidth), _ptr(thr), nt, out_shape=(ny, nx, nt), like=arr,
                  mem=_m.flags(f64, arr, thr))


def neighbourhood_members(input, halfwidth, statistic):
    """A spatial filter of every member of a cube (no counterpart in the reference, whose neighbourhood(vec3) pools the
    members into one field): (Y, X, E) -> (Y, X, E) float32, plane [..., e] = neighbourhood(input[..., e], halfwidth, statistic), without a
    permute of the cube.  Mean, Sum, Count, Min, Max, Std and Variance at any halfwidth >= 0, windows wider than the field included; invalid
    values (NaN, +-Inf) are left out and a window without a valid value gives NaN (Count: 0).

    input: numpy (float64 is cast on the device) or a torch CUDA tensor (then the result is one).  Median and RandomChoice raise ValueError:
    order statistics per member are not supported.  Quantile, a negative halfwidth: neighbourhood's errors.  A cube with a zero dimension
    gives an empty cube of that shape."""
    f64 = _wants_f64(input)
    arr = _m.field(input, 3, "input", f64)
    if halfwidth < 0:
        raise ValueError("Half width must be > 0")
    if statistic == Quantile:
        raise ValueError("Use neighbourhood_quantile for computing neighbourhood quantiles")
    for stat, name in ((Median, "Median"), (RandomChoice, "RandomChoice")):
        if statistic == stat:
            raise ValueError("neighbourhood_members does not compute the statistic %s: order statistics per member are not supported" % name)
    if statistic not in (Mean, Sum, Count, Min, Max, Std, Variance):
        raise ValueError("neighbourhood_members: unknown statistic")
    ny, nx, ne = _shape(arr)
    if ny * nx * ne == 0:
        return _m._empty_like_field((ny, nx, ne), arr)
    return _m.run(lib().gpp_neighbourhood_members, _ptr(arr), ny, nx, ne, int(halfwidth), int(statistic), out_shape=(ny, nx, ne), like=arr,
                  mem=_m.flags(f64, arr))


def calc_gradient_members(base, values, gradient_type, halfwidth, num_min=2, min_range=MV, default_gradient=0):
    """calc_gradient of every member of a cube (no counterpart in the reference): values (Y, X, E) -> (Y, X, E) float32,
    plane [..., e] = calc_gradient(base_e, values[..., e], ...), the layout plan.full_gradient_cube takes its gradients in.  base is (Y, X),
    one field shared by the members (elevation), or (Y, X, E), a field per member.  MinMax and LinearRegression; the checks and their
    messages are calc_gradient's.  numpy (float64 is cast on the device) or torch CUDA tensors (then the result is one)."""
    f64 = _wants_f64(base, values)
    base, values = _m.field(base, None, "base", f64), _m.field(values, 3, "values", f64)
    if halfwidth <= 0:
        raise ValueError("Halwidth cannot be <= 0; must be positive integer")
    if is_valid(min_range) and min_range < 0:
        raise ValueError("min_range must be >= 0")
    if num_min < 0:
        raise ValueError("num_min must be >= 0")
    bshape = _shape(base)
    if len(bshape) > 0 and bshape[0] == 0:
        raise ValueError("base input has no size")
    ny, nx, ne = _shape(values)
    if bshape not in ((ny, nx), (ny, nx, ne)):
        raise ValueError("base is not the same size as values")
    if gradient_type not in (MinMax, LinearRegression):
        raise ValueError("unknown gradient type")
    return _m.run(lib().gpp_calc_gradient_members, _ptr(base), 1 if len(bshape) == 2 else ne, _ptr(values), ny, nx, ne, int(gradient_type),
                  int(halfwidth), int(num_min), float(min_range), float(default_gradient), out_shape=(ny, nx, ne), like=values,
                  mem=_m.flags(f64, base, values))


def neighbourhood_ens(input, halfwidth, statistic):   # deprecated aliases (neighbourhood.cpp:541-552), with the reference's message
    future_deprecation_warning("neighbourhood_ens", "neighbourhood")
    return neighbourhood(input, halfwidth, statistic)


def neighbourhood_quantile_ens(input, quantile, halfwidth):
    future_deprecation_warning("neighbourhood_quantile_ens", "neighbourhood_quantile")
    return neighbourhood_quantile(input, quantile, halfwidth)


def neighbourhood_quantile_ens_fast(input, quantile, halfwidth, thresholds):
    future_deprecation_warning("neighbourhood_quantile_ens_fast", "neighbourhood_quantile_fast")
    return neighbourhood_quantile_fast(input, quantile, halfwidth, thresholds)


# ---- window statistics along the time axis (include/gridpp.h:1602-1611, src/api/window.cpp) -----------
_WINDOW_STATISTICS = (Mean, Min, Median, Max, Std, Variance, Sum, Count, RandomChoice)


def window(array, length, statistic, before=False, keep_missing=False, missing_edges=True):
    """src/api/window.cpp:6-156: the statistic over a window of `length` time steps for every (case, time) of a 2-D array; the
    window ends at the time step (before) or is centred on it (an odd length), clipped to the row.  Mean / Sum / Count are
    differences of the row's sequential float32 prefix sum, as in the reference; Count ignores keep_missing and missing_edges.
    keep_missing: NaN where the window holds a missing value; missing_edges: NaN where the window overshoots the row.
    (0, T) gives (0, 0) and (Y, 0) gives (Y, 0), as there.  Quantile and Unknown raise RuntimeError (the reference throws
    inside its loop; here before any device work)."""
    if length <= 0:
        raise ValueError("Length variable must be > 0")
    f64 = _wants_f64(array)
    arr = _m.field(array, 2, "array", f64)
    ny, nx = _shape(arr)
    if ny == 0 or nx == 0:
        return _empty_like_field((0, 0) if ny == 0 else (ny, 0), arr)
    if length % 2 == 0 and not before:
        raise ValueError("Length variable must be an odd number")
    if statistic not in _WINDOW_STATISTICS:
        raise RuntimeError("Internal error. Cannot compute statistic")
    return _m.run(lib().gpp_window, _ptr(arr), ny, nx, int(length), int(statistic), int(bool(before)), int(bool(keep_missing)),
                  int(bool(missing_edges)), out_shape=(ny, nx), like=arr, mem=_m.flags(f64, arr))


# ---- weather diagnostics (include/gridpp.h:49-67,1249-1367; src/api/humidity.cpp, pressure.cpp, qnh.cpp, wind.cpp) ------------------
# the `static const float` constants of include/gridpp.h:51-67, as SWIG hands them out: the float32 value as a Python float
MV_CML = -999.0
pi = float(np.float32(3.14159265))
lapse_rate = float(np.float32(0.0065))
standard_surface_temperature = float(np.float32(288.15))
gravit = float(np.float32(9.80665))
molar_mass = float(np.float32(0.0289644))
gas_constant_mol = float(np.float32(8.31447))
gas_constant_si = float(np.float32(287.05))


def _vectors_call(entry, args, names, size_checks):
    """An element-wise entry point on 1-D arrays of one length (host, or all torch CUDA tensors) -> an array of that length where they
    live.  size_checks: (i, j, message) in the reference's order."""
    f64 = _mem(*args) == _capi.MEM_HOST and _wants_f64(*args)   # (mixed memory is refused before the ranks are looked at)
    arrs = [_m.field(a, 1, n, f64) for a, n in zip(args, names)]
    for i, j, message in size_checks:
        if _shape(arrs[i]) != _shape(arrs[j]):
            raise ValueError(message)
    n = _shape(arrs[0])[0]
    if n == 0:
        return _empty_like_field((0,), arrs[0]) if _is_dev(arrs[0]) else np.zeros(0, np.float32)
    return _m.run(entry, *[_ptr(a) for a in arrs], n, out_shape=(n,), like=arrs[0], mem=_m.flags(f64, *arrs))


def _pointwise(entry, which, args, names, size_checks):
    """One diagnostic: every argument a scalar -> the host-only scalar form (a Python float back); otherwise 1-D arrays of one length
    (host, or all torch CUDA tensors) through the kernel.  size_checks: (i, j, message) in the reference's order."""
    if all(_ndim(a) == 0 for a in args):
        vals = (C.c_float * len(args))(*[float(a) for a in args])
        out = C.c_float(np.nan)
        check(lib().gpp_diagnostic_scalar(which, vals, len(args), C.byref(out)))
        return out.value
    return _vectors_call(entry, args, names, size_checks)


def dewpoint(temperature, relative_humidity):
    """src/api/humidity.cpp:5-32: dewpoint temperature [K] from temperature [K] and relative humidity [1]; never above the temperature
    (a relative humidity <= 0 returns the temperature).  Scalars or 1-D arrays."""
    return _pointwise(lib().gpp_dewpoint, _capi.DIAG_DEWPOINT, (temperature, relative_humidity), ("temperature", "relative_humidity"),
                      [(0, 1, "Temperature and relative_humidity vectors are not the same size")])


def relative_humidity(temperature, dewpoint):
    """src/api/humidity.cpp:33-90: relative humidity [1] from temperature and dewpoint temperature [K], by the saturation pressure
    table between 173.16 K and 368.16 K (clamped outside); 1 where temperature <= dewpoint.  Scalars or 1-D arrays."""
    return _pointwise(lib().gpp_relative_humidity, _capi.DIAG_RELATIVE_HUMIDITY, (temperature, dewpoint), ("temperature", "dewpoint"),
                      [(0, 1, "Temperature and dewpoint vectors are not the same size")])


def wetbulb(temperature, pressure, relative_humidity):
    """src/api/humidity.cpp:91-122: wetbulb temperature [K] from temperature [K], pressure [Pa] and relative humidity [1]; NaN for a
    relative humidity <= 0.  Scalars or 1-D arrays."""
    return _pointwise(lib().gpp_wetbulb, _capi.DIAG_WETBULB, (temperature, pressure, relative_humidity),
                      ("temperature", "pressure", "relative_humidity"),
                      [(0, 1, "Temperature and pressure vectors are not the same size"),
                       (0, 2, "Temperature and relative_humidity vectors are not the same size")])


def pressure(ielev, oelev, ipressure, itemperature=288.15):
    """src/api/pressure.cpp:5-26: the pressure [Pa] at elevation oelev [m] from the pressure at ielev and the temperature [K] there.
    Scalars (itemperature defaults to 288.15) or four 1-D arrays."""
    message = "pressure: Input arguments must be of the same size"
    return _pointwise(lib().gpp_pressure, _capi.DIAG_PRESSURE, (ielev, oelev, ipressure, itemperature),
                      ("ielev", "oelev", "ipressure", "itemperature"), [(0, 1, message), (0, 2, message), (0, 3, message)])


def sea_level_pressure(ps, altitude, temperature, rh=MV, dewpoint=MV):
    """src/api/pressure.cpp:28-93: surface pressure [Pa] reduced to sea level from the altitude [m], the 2 m temperature [K] and the
    relative humidity [1] or else the dewpoint temperature [K] (both NaN: dewpoint = temperature - 3).  Scalars (rh and dewpoint default
    to MV) or five 1-D arrays.  RuntimeError for a NaN altitude, a NaN temperature and unphysical values, tested in that order; the array
    form raises for the lowest offending index."""
    message = "slp: Input arguments must be of the same size"
    return _pointwise(lib().gpp_sea_level_pressure, _capi.DIAG_SEA_LEVEL_PRESSURE, (ps, altitude, temperature, rh, dewpoint),
                      ("ps", "altitude", "temperature", "rh", "dewpoint"), [(0, 1, message), (0, 2, message), (0, 3, message), (0, 4, message)])


def qnh(pressure, altitude):
    """src/api/qnh.cpp:6-41: QNH [Pa] from pressure [Pa] and altitude [m]; 0 for a pressure of 0.  Scalars or 1-D arrays."""
    return _pointwise(lib().gpp_qnh, _capi.DIAG_QNH, (pressure, altitude), ("pressure", "altitude"),
                      [(0, 1, "Pressure and altitude vectors are not the same size")])


def wind_speed(xwind, ywind):
    """src/api/wind.cpp:6-19.  No validity test: NaN propagates.  Scalars or 1-D arrays."""
    return _pointwise(lib().gpp_wind_speed, _capi.DIAG_WIND_SPEED, (xwind, ywind), ("xwind", "ywind"),
                      [(0, 1, "xwind and ywind must be of the same size")])


def wind_direction(xwind, ywind):
    """src/api/wind.cpp:20-37: the direction the wind comes from [degrees], 180 for (0, 0).  Scalars or 1-D arrays."""
    return _pointwise(lib().gpp_wind_direction, _capi.DIAG_WIND_DIRECTION, (xwind, ywind), ("xwind", "ywind"),
                      [(0, 1, "xwind and ywind must be of the same size")])


# ---- value transforms (include/gridpp.h:2345-2435, src/api/transform.cpp) -------------------------------------------------------------
def _typemap_shape(shape):
    """The shape the reference's output typemaps give an empty nested vector (swig/vector.i:332-339,515-525): every extent behind the
    first 0 is 0 -- (0, 1) -> (0, 0), (2, 0) -> (2, 0), (3, 3, 0) -> (3, 3, 0), (0, 3, 3) -> (0, 0, 0)."""
    out, dead = [], False
    for s in shape:
        out.append(0 if dead else s)
        dead = dead or s == 0
    return tuple(out)


class Transform:
    """include/gridpp.h:2345-2388: forward / backward of a scalar (host arithmetic, a Python float back) or of a 1-, 2- or 3-D array or
    torch CUDA tensor (one kernel, the same shape back as float32).  The base class's scalar forms return -1 (transform.cpp:7-12)."""
    _kind = None

    def _params(self):
        return 0.0, 0.0

    def forward(self, input):
        return self._apply(input, 0)

    def backward(self, input):
        return self._apply(input, 1)

    def _apply(self, value, backward):
        nd = _ndim(value)
        if nd == 0:
            if self._kind is None:
                return -1.0
            out = C.c_float(np.nan)
            check(self._scalar_entry(float(value), backward, C.byref(out)))
            return out.value
        if nd > 3:
            raise RuntimeError("input must be a scalar or have 1, 2 or 3 dimensions, got %d" % nd)
        dev, f64 = _is_dev(value), _wants_f64(value)
        v = _m.field(value, nd, "input", f64)
        shp = _shape(v)
        n = int(np.prod(shp))
        if n == 0:
            return _empty_like_field(_typemap_shape(shp), v) if dev else np.zeros(_typemap_shape(shp), np.float32)
        if self._kind is None:   # the vector forms call the virtual scalar one: -1 everywhere
            out = _empty_like_field(shp, v)
            out[...] = -1
            return out
        return _m.run(self._vector_entry, _ptr(v), n, backward, out_shape=shp, like=v, mem=_m.flags(f64, v))

    # the two C-ABI calls of _apply (a transform with other parameters than (p0, p1) overrides them)
    def _scalar_entry(self, value, backward, out):
        p0, p1 = self._params()
        return lib().gpp_transform_scalar(value, self._kind, backward, p0, p1, out)

    def _vector_entry(self, src, n, backward, dst, mem):
        p0, p1 = self._params()
        return lib().gpp_transform(src, n, self._kind, backward, p0, p1, dst, mem)


class Identity(Transform):
    """transform.cpp:180-185"""
    _kind = _capi.TRANSFORM_IDENTITY


class Log(Transform):
    """transform.cpp:85-96: log / exp of a valid value (forward(0) = -inf, a negative input gives NaN)"""
    _kind = _capi.TRANSFORM_LOG


class BoxCox(Transform):
    """transform.cpp:97-125: (value^threshold - 1) / threshold, log for threshold 0; inputs <= 0 count as 0.  The threshold is not
    validated."""
    _kind = _capi.TRANSFORM_BOXCOX

    def __init__(self, threshold):
        self._threshold = float(np.float32(threshold))

    def _params(self):
        return self._threshold, 0.0


class StartedBoxCox(Transform):
    """transform.cpp:126-154: no transformation between 0 and scaling_factor, a Box-Cox-like one with parameter threshold above."""
    _kind = _capi.TRANSFORM_STARTED_BOXCOX

    def __init__(self, threshold, scaling_factor):
        if not is_valid(threshold) or np.float32(threshold) <= 0:
            raise ValueError("threshold parameter must be > 0 in the started Box-Cox distribution")
        if not is_valid(scaling_factor) or np.float32(scaling_factor) <= 0:
            raise ValueError("Scaling factor parameter must be > 0 in the started Box-Cox distribution")
        self._threshold, self._scaling = float(np.float32(threshold)), float(np.float32(scaling_factor))

    def _params(self):
        return self._threshold, self._scaling


class Gamma(Transform):
    """transform.cpp:155-179: the cdf of the gamma distribution (shape, scale) at value + tolerance, rounded to float32, mapped to the
    standard normal quantile; backward the other way round, minus the tolerance.  Where the reference raises through Boost's error
    policies this returns IEEE values: forward gives NaN for value + tolerance < 0 and -inf / +inf where the float32
    cdf is 0 / 1, backward gives +inf where the float32 normal cdf is 1 (inputs above about 5.4).  Not part of the `gridpp` alias."""
    _kind = "gamma"   # not a GPP_TRANSFORM_* kind: the two entries below are its own

    def __init__(self, shape, scale, tolerance=0.01):
        if not is_valid(shape) or np.float32(shape) <= 0:
            raise ValueError("Shape parameter must be > 0 in the gamma distribution")
        if not is_valid(scale) or np.float32(scale) <= 0:
            raise ValueError("Scale parameter must be > 0 in the gamma distribution")
        if not is_valid(tolerance) or np.float32(tolerance) < 0:
            raise ValueError("Tolerance must be >= 0 in the gamma distribution")
        self._shape, self._scale, self._tolerance = (float(np.float32(v)) for v in (shape, scale, tolerance))

    def _scalar_entry(self, value, backward, out):
        return lib().gpp_gamma_transform_scalar(value, backward, self._shape, self._scale, self._tolerance, out)

    def _vector_entry(self, src, n, backward, dst, mem):
        return lib().gpp_gamma_transform(src, n, backward, self._shape, self._scale, self._tolerance, dst, mem)


def gamma_inv(levels, shape, scale):
    """src/api/distribution.cpp:5-33: the quantiles `levels` of gamma distributions, element by element: scale * x with
    P(shape, x) = level.  Three 1-D arrays (lists, numpy arrays, or all torch CUDA tensors: the result is then a tensor on that device)
    or three scalars (host arithmetic, a Python float back).  Level 0 gives 0; level 1 gives +inf, where the reference raises through
    Boost's overflow policy.  ValueError with the reference's texts for the lowest index with a level outside [0, 1],
    else a shape <= 0, else a scale <= 0 (NaN and infinities included).  The reference reads levels[i] and scale[i] up to len(shape)
    without comparing the lengths; here unequal lengths are a ValueError.  Not part of the `gridpp` alias."""
    args = (levels, shape, scale)
    if all(_ndim(a) == 0 for a in args):
        out = C.c_float(np.nan)
        check(lib().gpp_gamma_inv_scalar(float(levels), float(shape), float(scale), C.byref(out)))
        return out.value
    message = "gamma_inv: levels, shape and scale must be of the same size"
    return _vectors_call(lib().gpp_gamma_inv, args, ("levels", "shape", "scale"), [(0, 1, message), (1, 2, message)])


# ---- verification scores (include/gridpp.h:103-110; src/api/metric_optimizer.cpp:185-244, neighbourhood_score.cpp) ----
Ets, Ts, Kss, Pc, Bias, Hss = 0, 1, 20, 30, 40, 50
_METRICS = (Ets, Ts, Kss, Pc, Bias, Hss)


def _metric(metric):
    if metric not in _METRICS:
        raise ValueError("Unknown metric")
    return int(metric)


def _ref_fcst(ref, fcst, f64=False):
    """ref and fcst as 1-D fields (a device tensor of another rank raises the score functions' own text)"""
    return (_m.field(ref, 1, "ref", f64, dev_message="ref must have 1 dimension"),
            _m.field(fcst, 1, "fcst", f64, dev_message="fcst must have 1 dimension"))


def calc_score(*args):
    """src/api/metric_optimizer.cpp:185-244, the three overloads of include/gridpp.h:

    calc_score(a, b, c, d, metric): the score of a contingency table, host arithmetic with the reference's float / double promotions.
    calc_score(ref, fcst, threshold, metric) and calc_score(ref, fcst, threshold, fthreshold, metric): the table of the first
    len(fcst) elements (counted on the GPU; numpy arrays or torch CUDA tensors), then the same rule.  A NaN ref is counted nowhere, a NaN
    fcst as c or d, and every count stops at 2**24, all as in the reference.  The five-argument forms are told apart by whether the first
    argument is a scalar.  A ref shorter than fcst is read out of bounds by the reference; here it raises ValueError("ref and fcst not the
    same size").  Empty vectors need no GPU: Bias is 1, every other metric NaN."""
    if len(args) not in (4, 5):
        raise TypeError("calc_score takes 4 or 5 arguments")
    out = C.c_float()
    if len(args) == 5 and not _is_dev(args[0]) and np.ndim(args[0]) == 0:
        a, b, c, d, metric = args
        check(lib().gpp_calc_score_table(float(a), float(b), float(c), float(d), _metric(metric), C.byref(out)))
        return out.value
    if len(args) == 4:
        ref, fcst, threshold, metric = args
        fthreshold = threshold
    else:
        ref, fcst, threshold, fthreshold, metric = args
    metric = _metric(metric)
    ref, fcst = _ref_fcst(ref, fcst)
    n = _shape(fcst)[0]
    if _shape(ref)[0] < n:
        raise ValueError("ref and fcst not the same size")
    mem = _m.flags(False, ref, fcst) if n else _capi.MEM_HOST
    check(lib().gpp_calc_score(_ptr(ref), _ptr(fcst), n, float(threshold), float(fthreshold), metric, C.byref(out), mem))
    return out.value


def neighbourhood_score(grid, points, fcst, ref, half_width, metric, threshold):
    """src/api/neighbourhood_score.cpp:6-60: the score of every grid cell over the (2 half_width + 1)^2 cells around it (clipped to the
    grid): the observations `ref` at `points` are gridded (gridding_nearest, min_num 1, Mean), a cell counts where that and `fcst` are
    both finite, and the fractions of a / b / c / d cells of the window go through calc_score.  fcst: a numpy array or a torch CUDA tensor
    (the result is then one too); ref: a host vector.  Checks in the reference's order: "Grid size is not the same as forecast values",
    "half_width must be greater than 0", "Unknown metric", "Points size is not the same as values".  An empty grid gives an empty array."""
    f64 = _wants_f64(fcst)
    f = _m.field(fcst, 2, "fcst", f64)
    shp = _shape(f)
    ny, nx = grid.size()
    if shp[0] != 0 and tuple(shp) != (ny, nx):                 # src/api/util.cpp:427-429
        raise ValueError("Grid size is not the same as forecast values")
    if half_width <= 0:
        raise ValueError("half_width must be greater than 0")
    metric = _metric(metric)
    r = _m.field(ref, 1, "ref")
    if r.shape[0] != points.size():
        raise ValueError("Points size is not the same as values")
    if ny * nx == 0:
        return _empty_like_field((ny, nx), f)
    if shp[0] == 0:   # (the reference reads fcst[0] of an empty vector here)
        raise ValueError("Grid size is not the same as forecast values")
    return _m.run(lib().gpp_neighbourhood_score, grid._h, points._h, _ptr(f), _ptr(r), int(half_width), metric, float(threshold),
                  out_shape=(ny, nx), like=f, mem=_m.flags(f64, f))


# ---- the Fractions Skill Score (no counterpart in the reference) ----
FssResult = collections.namedtuple("FssResult", ["fss", "fbs", "fbs_worst", "cells"])


def _fss_value(fbs, fbs_worst):
    """GPP_FSS_VALUE of include/gridpp_hip.h, elementwise: 1 - fbs / fbs_worst in float64, NaN where fbs_worst == 0"""
    fbs, fbs_worst = np.asarray(fbs, np.float64), np.asarray(fbs_worst, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(fbs_worst == 0, np.nan, 1.0 - fbs / fbs_worst)


def fractions_skill_score(fcst, ref, thresholds, halfwidths, comparison_operator=Gt):
    """The Fractions Skill Score (Roberts & Lean 2008; for an ensemble the neighbourhood ensemble probability of Schwartz & Sobash 2017)
    of `fcst` against `ref` for every threshold and every half width from one call (no counterpart in the reference):
    FssResult(fss, fbs, fbs_worst, cells), host numpy whatever the inputs are -- fss, fbs and fbs_worst float64 of shape (T, H), cells
    int64 of shape (H,).

    fcst: (Y, X), or an ensemble cube (Y, X, E); ref: (Y, X); numpy arrays of any dtype, or both torch CUDA tensors.  thresholds: a 1-D
    host sequence (+-Inf allowed, NaN is not); halfwidths: a 1-D host sequence of ints >= 0; comparison_operator: Lt, Leq, Gt or Geq
    (Gt is what calc_score and neighbourhood_score use).

    A cell counts where ref is valid (not NaN, not +-Inf) and fcst has a valid member; m = its valid members, k = those with
    `member op threshold`, o = `ref op threshold`.  Over the window [y +- h] x [x +- h] clipped to the grid (the window of
    neighbourhood) n, M, K, O are the exact sums of 1, m, k, o over the counting cells.  Every cell with n > 0 contributes, whether it
    counts itself or not: Ff = K / M, Fo = O / n, fbs += (Ff - Fo)^2, fbs_worst += Ff^2 + Fo^2, in float64; cells[h] is their number.
    fss = 1 - fbs / fbs_worst, NaN where fbs_worst == 0 (no event in either field).  Ff is the POOLED member fraction of the window: the
    mean of the per-cell ensemble probabilities k / m wherever every counting cell has the same number of valid members; where they
    differ, a cell weighs by the members it has.

    To pool over cases (dates), add the sums, not the scores: 1 - sum(fbs) / sum(fbs_worst).

    The result is bit-identical from call to call.  Errors, all before any device work and in this order: RuntimeError for a wrong number
    of dimensions; ValueError where ref is not (Y, X) of fcst, thresholds or halfwidths are not 1-D, a threshold is NaN, a half width is
    no integer or negative, the operator is none of the four, or one field is a device tensor and the other is not.  T == 0, H == 0 and an empty field
    need no device (an empty field: zeros, NaN fss, cells == 0; without a threshold cells is 0 too)."""
    f, ny, nx, ne, is3d, _ = _field23(fcst, "fcst")
    r = _m.field(ref, 2, "ref")
    if _shape(r) != (ny, nx) and not (ny * nx == 0 and int(np.prod(_shape(r))) == 0):
        raise ValueError("fractions_skill_score: ref must have the shape (Y, X) of fcst")
    thr, hws = np.asarray(thresholds), np.asarray(halfwidths)
    if thr.ndim != 1:
        raise ValueError("fractions_skill_score: thresholds must have 1 dimension")
    if hws.ndim != 1:
        raise ValueError("fractions_skill_score: halfwidths must have 1 dimension")
    thr = np.ascontiguousarray(thr, np.float32)
    if np.isnan(thr).any():
        raise ValueError("fractions_skill_score: a threshold is NaN")
    if hws.size and hws.dtype.kind not in "iub":
        raise ValueError("fractions_skill_score: halfwidths must be integers")
    if hws.size and hws.min() < 0:
        raise ValueError("Half width must be > 0")
    if comparison_operator not in (Lt, Leq, Gt, Geq):
        raise ValueError("Invalid comparison operator")
    mem = _m.flags(False, f, r)
    hws = np.ascontiguousarray(np.minimum(hws, 2 ** 31 - 1), np.int32)   # (no window is wider than the field)
    nt, nh = int(thr.size), int(hws.size)
    fbs, worst, cells = np.zeros((nt, nh), np.float64), np.zeros((nt, nh), np.float64), np.zeros(nh, np.int64)
    if nt and nh and ny * nx * ne:
        check(lib().gpp_fractions_skill_score(_ptr(f), _ptr(r), ny, nx, ne, is3d, _ptr(thr), nt, _ptr(hws), nh, int(comparison_operator),
                                              _ptr(fbs), _ptr(worst), _ptr(cells), mem))
    return FssResult(_fss_value(fbs, worst), fbs, worst, cells)


# ---- the optimal forecast threshold (src/api/metric_optimizer.cpp:105-184) ----
def _optimizer_vectors(ref, fcst):
    """-> ref, fcst, f64: numpy arrays (float64 ones of 2**20 values and more are cast on the device) or torch CUDA tensors"""
    f64 = _mem(ref, fcst) == _capi.MEM_HOST and _wants_f64(ref, fcst)   # (mixed memory is refused before the ranks are looked at)
    return _ref_fcst(ref, fcst, f64) + (f64,)


def get_optimal_threshold(ref, fcst, threshold, metric):
    """The forecast threshold x that maximises calc_score(ref, fcst, threshold, x, metric), as DESIGN.md 4.13 defines it: the score is
    constant between two neighbouring values of fcst, so every plateau [u_k, u_k+1) of the distinct finite values u_0 < ... < u_m-1 is
    evaluated (one sort and one sweep on the GPU) and the result is the midpoint of the lowest run of plateaus with the largest valid
    score (its lower end where the midpoint would round up to the next plateau).  NaN with the reference's filters
    (src/api/metric_optimizer.cpp:165-182): no valid score, a best score <= 0.0001, or one within 0.001 of the score at u_0 or u_m-1; also
    for empty vectors (no GPU needed) and without a finite fcst.  The reference minimises with Boost's brent_find_minima, which ends
    somewhere on whichever plateau it reaches: this result is never worse and is defined, but it is not the reference's number, so the
    name is not part of the `gridpp` alias.  ref, fcst: numpy arrays or torch CUDA tensors; a float comes back.  ValueError("Unknown
    metric"); a ref shorter than fcst is ValueError("ref and fcst not the same size"), as for calc_score."""
    metric = _metric(metric)
    ref, fcst, f64 = _optimizer_vectors(ref, fcst)
    n = _shape(fcst)[0]
    if _shape(ref)[0] < n:
        raise ValueError("ref and fcst not the same size")
    out = C.c_float(np.nan)
    mem = _m.flags(f64, ref, fcst) if n else _capi.MEM_HOST
    check(lib().gpp_get_optimal_threshold(_ptr(ref), _ptr(fcst), n, float(threshold), metric, C.byref(out), mem))
    return out.value


def metric_optimizer_curve(ref, fcst, thresholds, metric):
    """src/api/metric_optimizer.cpp:105-127 on get_optimal_threshold above: -> (curve_ref, curve_fcst), two float32 numpy arrays.  For
    every threshold t, in order, whose optimal forecast threshold x is valid, x goes to curve_ref and t to curve_fcst (the reference's
    naming).  One sort serves all thresholds.  ValueError("ref and fcst not the same size") unless both have the same length; empty
    thresholds give two empty arrays and need no GPU.  Not part of the `gridpp` alias."""
    metric = _metric(metric)
    ref, fcst, f64 = _optimizer_vectors(ref, fcst)
    n = _shape(fcst)[0]
    if _shape(ref)[0] != n:
        raise ValueError("ref and fcst not the same size")
    thresholds = _vec(thresholds.cpu().numpy() if _is_dev(thresholds) else thresholds, 1, "thresholds")   # a host vector whatever ref and fcst are
    T = thresholds.shape[0]
    curve_ref, curve_fcst, count = np.empty(T, np.float32), np.empty(T, np.float32), C.c_int(0)
    if T and n:
        check(lib().gpp_metric_optimizer_curve(_ptr(ref), _ptr(fcst), n, _ptr(thresholds), T, metric, _ptr(curve_ref), _ptr(curve_fcst),
                                               C.byref(count), _m.flags(f64, ref, fcst)))
    return curve_ref[:count.value].copy(), curve_fcst[:count.value].copy()


# ---- util (include/gridpp.h:1454-1482, src/api/util.cpp) ---------------------------------------------
def _rows_array(array, maxdim):
    """calc_statistic / calc_quantile input: a host array or a torch CUDA tensor -> C-contiguous float32 of 1 .. maxdim dimensions"""
    a = _m.field(array)
    if not 1 <= len(_shape(a)) <= maxdim:
        raise RuntimeError("array must have %s dimensions" % ("1 or 2" if maxdim == 2 else "1, 2 or 3"))
    return a


def _rows_call(entry, a, rows, *args, mem):
    """One value per row of `a` where it lives (none for no rows); a 1-D input -> a Python float."""
    out = _m.run(entry, _ptr(a), rows, *args, out_shape=(rows,), like=a, mem=mem) if rows else _empty_like_field((0,), a)
    if len(_shape(a)) != 1:
        return out
    return float(out[0].item()) if _is_dev(out) else float(out[0])


def calc_statistic(array, statistic):
    """gridpp::calc_statistic for a vector (-> float) or a 2-D array (-> one value per row); host arrays or torch CUDA tensors."""
    a = _rows_array(array, 2)
    shp = _shape(a)
    rows = 1 if len(shp) == 1 else shp[0]
    return _rows_call(lib().gpp_calc_statistic, a, rows, shp[-1], int(statistic), mem=_m.flags(False, a))


def calc_quantile(array, quantile):
    """gridpp::calc_quantile: (vec, q) -> float, (vec2, q) -> vec, (vec3, vec2 q) -> vec2; host arrays or torch CUDA tensors (a
    quantile field beside a device-resident cube may be either and is uploaded when it is a host array)."""
    a = _rows_array(array, 3)
    shp = _shape(a)
    dev = _is_dev(a)
    if dev:
        import torch
        q = _m.field(quantile)
        if not _is_dev(q):
            q = torch.from_numpy(q).to(a.device)
    else:
        _mem(a, quantile)   # (a device-resident quantile beside a host array: _mem's error)
        q = _m.field(quantile)
    if len(shp) == 3:
        if _shape(q) != shp[:2]:
            raise ValueError("Dimension mismatch between array and quantile")
        if shp[0] * shp[1] == 0:
            return np.zeros((0, 0), np.float32)
        rows = shp[0] * shp[1]
        return _m.run(lib().gpp_calc_quantile, _ptr(a), rows, shp[2], _ptr(q), rows, out_shape=(rows,), like=a,
                      mem=_m.flags(False, a, q)).reshape(shp[:2])
    qq = q.reshape(1)
    return _rows_call(lib().gpp_calc_quantile, a, 1 if len(shp) == 1 else shp[0], shp[-1], _ptr(qq), 1, mem=_m.flags(False, a, qq))


def _levels(quantiles):
    """the levels of calc_quantiles / quantile_mapping_curves: a 1-D sequence -> host float32 (a device tensor is copied to the host)"""
    return _vec(quantiles.cpu().numpy() if _is_dev(quantiles) else quantiles, 1, "quantiles")


def calc_quantiles(array, quantiles):
    """Many quantiles of every row in one call: (N,) -> (Q,), (R, N) -> (R, Q), (Y, X, N) -> (Y, X, Q), where out[..., j] holds exactly the
    bits of calc_quantile(row, quantiles[j]).  Host arrays or torch CUDA tensors; the result lives where the input does.  `quantiles` is a
    1-D sequence on the host (a device tensor is copied there), in any order, repeats allowed; a NaN level gives NaN.  Rows of up to 8192
    values are sorted once in LDS and every level picked out of the sorted row.  RuntimeError for an array that has not
    1, 2 or 3 dimensions, ValueError for a level below 0 or above 1.  No counterpart in the reference: not part of the `gridpp` alias."""
    a = _rows_array(array, 3)
    q = _levels(quantiles)
    if np.any((q < 0) | (q > 1)):
        raise ValueError("calc_quantiles: Quantiles must be between 0 and 1 inclusive")
    shp = _shape(a)
    rows, nq = int(np.prod(shp[:-1], dtype=np.int64)), q.shape[0]
    if rows == 0 or nq == 0:
        return _empty_like_field(shp[:-1] + (nq,), a)
    return _m.run(lib().gpp_calc_quantiles, _ptr(a), rows, shp[-1], _ptr(q), nq, out_shape=(rows, nq), like=a,
                  mem=_m.flags(False, a)).reshape(shp[:-1] + (nq,))


def quantile_mapping_curves(ref, fcst, quantiles):
    """One quantile-mapping curve per cell -> (curve_ref, curve_fcst) for cubes ref (Y, X, Tr) and fcst (Y, X, Tf): (Y, X, Q) each, with
    curve_*[y, x, j] = calc_quantile(that cell's values, quantiles[j]); the pair is what apply_curve(fcst (Y, X), curve_ref, curve_fcst, ...)
    takes, and it lives where the cubes do (host arrays or torch CUDA tensors).  Tr and Tf may differ.

    Unlike the 1-D quantile_mapping_curve these are TRUE quantiles of each cell's valid values (calc_quantile's interpolation between order
    statistics).  The reference's 1-D function with quantiles indexes into the inputs as given (src/api/quantile_mapping.cpp:41-42), and the
    1-D function here reproduces that.  ValueError: first two dimensions that differ, host and device inputs mixed, empty quantiles (the
    sorted-rows form of the 1-D function is not built per cell), a level that is NaN or outside [0, 1] (a NaN knot is useless in a curve).
    No counterpart in the reference: not part of the `gridpp` alias."""
    r, f = _m.field(ref, 3, "ref"), _m.field(fcst, 3, "fcst")
    if _shape(r)[:2] != _shape(f)[:2]:
        raise ValueError("quantile_mapping_curves: ref and fcst must have the same first two dimensions")
    _mem(r, f)
    q = _levels(quantiles)
    if q.shape[0] == 0:
        raise ValueError("quantile_mapping_curves: empty quantiles: the sorted-rows form is not built")
    if not np.all((q >= 0) & (q <= 1)):   # (NaN fails)
        raise ValueError("Quantiles must be >= 0 and <= 1")
    return calc_quantiles(r, q), calc_quantiles(f, q)


def _rank_rows(a):
    """(rows, len) of an array whose last axis is the row"""
    shp = _shape(a)
    return int(np.prod(shp[:-1], dtype=np.int64)), shp[-1]


def calc_ranks(array):
    """The rank of every value within its row (the last axis): (N,), (R, N) or (Y, X, N) -> int32 of the same shape.  For a valid (finite)
    element rank[i] = #{valid j : a[j] < a[i]} + #{valid j < i : a[j] == a[i]}: values compare numerically (-0.0 == +0.0) and equal values are
    ordered by position, lower index first -- numpy.argsort(kind="stable") on the valid values of the row.  An invalid element has rank -1.
    Host arrays or torch CUDA tensors; the result lives where the input does.  RuntimeError for an array that has not 1, 2 or
    3 dimensions.  No counterpart in the reference: not part of the `gridpp` alias."""
    a = _rows_array(array, 3)
    rows, n = _rank_rows(a)
    if rows * n == 0:
        return _empty_like_field(_shape(a), a, np.int32)
    L = lib()
    return _m.run(lambda p, r, l, out, mem: L.gpp_calc_ranks(p, r, l, out, None, mem), _ptr(a), rows, n, out_shape=_shape(a), like=a,
                  mem=_m.flags(False, a), dtype=np.int32)


def sort_rows(array):
    """Every row (the last axis) in the order of calc_ranks: out[..., calc_ranks(a)[..., i]] = a[..., i] with the bits of a[..., i] kept (a
    -0.0 stays -0.0, equal values keep their order), and NaN in the slots from N, the number of valid values, on.  float32 of the input's
    shape, where the input lives.  No counterpart in the reference: not part of the `gridpp` alias."""
    a = _rows_array(array, 3)
    rows, n = _rank_rows(a)
    if rows * n == 0:
        return _empty_like_field(_shape(a), a)
    L = lib()
    return _m.run(lambda p, r, l, out, mem: L.gpp_calc_ranks(p, r, l, None, out, mem), _ptr(a), rows, n, out_shape=_shape(a), like=a,
                  mem=_m.flags(False, a))


def reorder_by_ranks(values, template):
    """Ensemble copula coupling (ECC-Q; the Schaake shuffle when `template` is a historical sample): member i receives the value of `values`
    whose rank equals the rank of template member i.  Two arrays of the same shape, (N,), (R, N) or (Y, X, N); out[..., i] =
    sort_rows(values)[..., calc_ranks(template)[..., i]], bit for bit, and NaN where the template's value is invalid or its rank is not below the
    number of valid entries of the `values` row.  Ties in the template are broken by position (lower index first), not at random.  The result
    lives where the inputs do.  RuntimeError for an array that has not 1, 2 or 3 dimensions, ValueError for shapes that differ.
    No counterpart in the reference: not part of the `gridpp` alias."""
    v, t = _rows_array(values, 3), _rows_array(template, 3)
    if _shape(v) != _shape(t):
        raise ValueError("reorder_by_ranks: values and template must have the same shape")
    _mem(v, t)
    rows, n = _rank_rows(v)
    if rows * n == 0:
        return _empty_like_field(_shape(v), v)
    return _m.run(lib().gpp_reorder_by_ranks, _ptr(v), _ptr(t), rows, n, out_shape=_shape(v), like=v, mem=_m.flags(False, v, t))


def calc_crps(ensemble, ref):
    """The continuous ranked probability score of every row (the last axis) of `ensemble` against `ref`, whose shape is the ensemble's without
    its last axis: CRPS = (1/N) sum_k |x_(k) - y| - (1/N^2) sum_k (2k - N + 1) x_(k) over the N sorted valid members, the rank form of
    (1/N) sum |x_i - y| - (1/(2 N^2)) sum sum |x_i - x_j|.  Both sums are taken in double and cast to float32 last; NaN when a row has no valid
    member or y is not finite.  float32 of ref's shape, where the inputs live.  RuntimeError for an ensemble that has not 1, 2
    or 3 dimensions, ValueError for a `ref` of another shape.  No counterpart in the reference: not part of the `gridpp` alias."""
    e = _rows_array(ensemble, 3)
    yshape = _shape(ref) if _is_dev(ref) else np.shape(ref)   # (before the conversion: a scalar beside a vector comes back as one value)
    y = _m.field(ref)
    if tuple(yshape) != _shape(e)[:-1]:
        raise ValueError("calc_crps: ref must have the shape of ensemble without its last axis")
    _mem(e, y)
    rows, n = _rank_rows(e)
    if rows == 0:
        return _empty_like_field(yshape, e)
    out = _m.run(lib().gpp_calc_crps, _ptr(e), _ptr(y), rows, n, out_shape=(rows,), like=e, mem=_m.flags(False, e, y))
    return out.reshape(yshape)


def _even_quantiles(values, num, only_valid):
    dev = _is_dev(values)
    v = _m.field(values).reshape(-1)
    n = int(v.numel()) if dev else v.size
    out = np.empty(max(int(num), 1) if n else 1, np.float32)
    if num > 0 and n > 0 and num >= n:
        out = np.empty(n, np.float32)
    cnt = C.c_int(0)
    if dev:
        dout = _empty_like_field(out.size, v)
        check(lib().gpp_calc_even_quantiles(_ptr(v), n, int(num), int(only_valid), _ptr(dout), C.byref(cnt), _m.flags(False, v)))
        return dout[:cnt.value].cpu().numpy()
    check(lib().gpp_calc_even_quantiles(_ptr(v), n, int(num), int(only_valid), _ptr(out), C.byref(cnt), _m.flags(False, v)))
    return out[:cnt.value].copy()


def calc_even_quantiles(values, num):
    """gridpp::calc_even_quantiles (src/api/util.cpp:261-338)."""
    return _even_quantiles(values, num, 0)


def get_neighbourhood_thresholds(input, num_thresholds):
    """gridpp::get_neighbourhood_thresholds for 2-D / 3-D input (src/api/neighbourhood.cpp:243-295)."""
    if num_thresholds <= 0:
        raise ValueError("num_thresholds must be > 0")
    return _even_quantiles(input, num_thresholds, 1)


# ---- ensemble OI (include/gridpp.h:263-294, src/api/oi_ensi.cpp) ----------------------------------------
def optimal_interpolation_ensi(bgrid, background, points, pobs, psigmas, pbackground, structure, max_points, allow_extrapolation=True):
    """gridpp::optimal_interpolation_ensi, Grid (background (Y, X, E)) and Points (background (N, E)) overloads."""
    if max_points < 0:
        raise ValueError("max_points must be >= 0")
    if not isinstance(bgrid, (Grid, Points)) or not isinstance(points, Points):
        raise TypeError("bgrid must be a Grid or Points, points a Points")
    nd = 3 if isinstance(bgrid, Grid) else 2
    S = points.size()
    f64 = S > 0 and _wants_f64(background)
    background = _m.field(background, nd, "background", f64)
    if S == 0:   # src/api/oi_ensi.cpp:48-50,135-137: returns the background before any other check
        return background.clone() if _is_dev(background) else background.copy()
    if bgrid.get_coordinate_type() != points.get_coordinate_type():
        raise ValueError("Both background and observations points must be of same coordinate type (lat/lon or x/y)")
    shape = _out_shape(bgrid)
    if nd == 3 and shape[0] * shape[1] == 0:
        raise ValueError("Grid size cannot be zero")
    if _shape(background)[:nd - 1] != shape:
        raise ValueError("Input field is not the same size as the grid")
    E = _shape(background)[-1]
    pobs, psigmas = _m.field(pobs, 1, "obs", f64), _m.field(psigmas, 1, "sigmas", f64)
    pbackground = _m.field(pbackground, 2, "background_at_points", f64)
    if _shape(pobs)[0] != S:
        raise ValueError("Observations and points size mismatch")
    if _shape(psigmas)[0] != S:
        raise ValueError("Sigmas and points size mismatch")
    if _shape(pbackground)[0] != S:
        raise ValueError("Background and points size mismatch")
    if _shape(pbackground)[1] != E:
        raise ValueError("Ensemble members in gridded background is not the same as in the point background")
    mem = _m.flags(f64, background, pobs, psigmas, pbackground)
    out = _empty_like_field(_shape(background), background)
    check(lib().gpp_optimal_interpolation_ensi(bgrid._h, _ptr(background), int(E), points._h, _ptr(pobs), _ptr(psigmas),
                                               _ptr(pbackground), _structure(structure), int(max_points),
                                               int(bool(allow_extrapolation)), _ptr(out), mem))
    _ensi_warnings()
    return out


def ensi_last_stats():
    """cells, the grid points the last optimal_interpolation_ensi left at their background values (singular / non-finite E x E system:
    the reference's num_condition_warning, oi_ensi.cpp:153,386-390), its second counter (always 0 here) and the kernel time"""
    s = _capi.gpp_ensi_stats()
    check(lib().gpp_ensi_last_stats(C.byref(s)))
    return dict(cells=s.cells, condition_passthrough=s.condition_passthrough, real_part_passthrough=s.real_part_passthrough, kernel_ms=s.kernel_ms)


def _ensi_warnings():
    """the two warnings the reference prints at the end of optimal_interpolation_ensi (oi_ensi.cpp:557-566)"""
    s = ensi_last_stats()
    if s["condition_passthrough"] > 0:
        warning("Condition number error in %d points. Using raw values in those points." % s["condition_passthrough"])
    if s["real_part_passthrough"] > 0:
        warning("Could not find the real part of W in %d points. Using raw values in those points." % s["real_part_passthrough"])


def _ensi_multi(variant, name, bgrid, bratios, background, background_corr, points, pobs, pratios, pbackground, pbackground_corr,
                structure, max_points, allow_extrapolation):
    """Shared body of the optimal_interpolation_ensi_multi_* mirrors (validation as src/api/oi_ensi_multi.cpp:341-362)."""
    if max_points < 0:
        raise ValueError("max_points must be >= 0")
    if not isinstance(bgrid, (Grid, Points)) or not isinstance(points, Points):
        raise TypeError("bgrid must be a Grid or Points, points a Points")
    nd = 3 if isinstance(bgrid, Grid) else 2
    S = points.size()
    background = _m.field(background, nd, "background")
    if S == 0:
        return background.clone() if _is_dev(background) else background.copy()
    if bgrid.get_coordinate_type() != points.get_coordinate_type():
        raise ValueError("Both background and observations points must be of same coorindate type (lat/lon or x/y)")
    shape = _out_shape(bgrid)
    if nd == 3 and shape[0] * shape[1] == 0:
        raise ValueError("Grid size cannot be zero")
    if _shape(background)[:nd - 1] != shape:
        raise ValueError("Input background field is not the same size as the grid")
    E = _shape(background)[-1]
    corr = variant != 2
    if corr:
        background_corr = _m.field(background_corr, nd, "background_corr")
        if _shape(background_corr) != _shape(background):
            raise ValueError("Input background_corr field is not the same size as the grid")
        pbackground_corr = _m.field(pbackground_corr, 2, "pbackground_corr")
        if _shape(pbackground_corr)[0] != S:
            raise ValueError("Background_corr and points size mismatch")
    bratios = _m.field(bratios, nd - 1, "bratios")
    if _shape(bratios) != shape:
        raise ValueError("Bratios and grid size mismatch")
    pobs = _m.field(pobs, 1 if variant == 3 else 2, "pobs")
    pratios = _m.field(pratios, 1, "pratios")
    pbackground = _m.field(pbackground, 2, "pbackground")
    if _shape(pobs)[0] != S:
        raise ValueError("Observations and points exception mismatch")
    if _shape(pratios)[0] != S:
        raise ValueError("Pratios and points size mismatch")
    if _shape(pbackground)[0] != S:
        raise ValueError("Background and points size mismatch")
    if _shape(pbackground)[1] != E or (variant != 3 and _shape(pobs)[1] != E) or (corr and _shape(pbackground_corr)[1] != E):
        raise ValueError("Ensemble members in gridded background is not the same as in the point fields")
    args = [bratios, background, pobs, pratios, pbackground] + ([background_corr, pbackground_corr] if corr else [])
    mem = _m.flags(False, *args)
    out = _empty_like_field(_shape(background), background)
    check(lib().gpp_optimal_interpolation_ensi_multi(int(variant), bgrid._h, _ptr(bratios), _ptr(background),
                                                     _ptr(background_corr) if corr else None, int(E), points._h, _ptr(pobs), _ptr(pratios),
                                                     _ptr(pbackground), _ptr(pbackground_corr) if corr else None, _structure(structure),
                                                     int(max_points), int(bool(allow_extrapolation)), _ptr(out), mem))
    return out


def optimal_interpolation_ensi_multi_ebe(bgrid, bratios, background, background_corr, obs_points, pobs, pratios, pbackground,
                                         pbackground_corr, structure, max_points, allow_extrapolation=True):
    """gridpp::optimal_interpolation_ensi_multi_ebe (include/gridpp.h:311-322,373-384): ensemble-based correlations, member by member."""
    return _ensi_multi(1, "ebe", bgrid, bratios, background, background_corr, obs_points, pobs, pratios, pbackground, pbackground_corr,
                       structure, max_points, allow_extrapolation)


def optimal_interpolation_ensi_multi_ebesc(bgrid, bratios, background, obs_points, pobs, pratios, pbackground, structure, max_points,
                                           allow_extrapolation=True):
    """gridpp::optimal_interpolation_ensi_multi_ebesc (include/gridpp.h:336-345,398-407): static correlations, member by member."""
    return _ensi_multi(2, "ebesc", bgrid, bratios, background, None, obs_points, pobs, pratios, pbackground, None, structure, max_points,
                       allow_extrapolation)


def optimal_interpolation_ensi_multi_utem(bgrid, bratios, background, background_corr, obs_points, pobs, pratios, pbackground,
                                          pbackground_corr, structure, max_points, allow_extrapolation=True):
    """gridpp::optimal_interpolation_ensi_multi_utem (include/gridpp.h:360-371,421-432): ensemble mean first, then the analysis ensemble."""
    return _ensi_multi(3, "utem", bgrid, bratios, background, background_corr, obs_points, pobs, pratios, pbackground, pbackground_corr,
                       structure, max_points, allow_extrapolation)


def ensi_last_kernel_ms():
    ms = C.c_float(0)
    check(lib().gpp_ensi_last_kernel_ms(C.byref(ms)))
    return ms.value


def ensi_set_convergence(to_convergence):
    """True: the per-cell Jacobi sweeps of optimal_interpolation_ensi run to convergence (about twice the time);
    False (default): they stop early and a perturbation series supplies the rest."""
    check(lib().gpp_ensi_set_convergence(1 if to_convergence else 0))


def set_path_override(name, value):
    """The library's one test / A-B hook: `name` = a GPP_* path switch (they select between implementations with identical results),
    `value` = its setting as a string, None clears it.  The library reads no environment variable itself."""
    check(lib().gpp_set_path_override(str(name).encode(), None if value is None else str(value).encode()))


def active_overrides():
    """Names of the GPP_* path switches that are set (they select implementations, never results)."""
    buf = C.create_string_buffer(4096)
    n = lib().gpp_active_overrides(buf, len(buf))
    return [s for s in buf.value.decode().split(",") if s] if n > 0 else []


def release_workspaces():
    """Frees the large device workspaces this thread keeps between calls."""
    check(lib().gpp_release_workspaces())


# ---- the typemap test helpers of the reference (src/api/swig.cpp:6-100, include/gridpp.h:1680-1702): they exist so that
# tests/test_swig.py can pin the binding layer -- element types of results, accepted input types, ndim checks, zero-size
# dimensions.  Here they exercise the same conversion helper (_vec) every entry point of this mirror goes through.
_SWIG_DEFAULT = -1          # swig_default_value


def _ivec(a, ndim, name="array"):
    arr = np.ascontiguousarray(np.asarray(a), dtype=np.int32)
    if arr.ndim != ndim:
        if arr.size == 0 and arr.ndim <= ndim:
            return arr.reshape((0,) * ndim)
        raise RuntimeError("%s must have %d dimensions, got %d" % (name, ndim, arr.ndim))
    return arr


def _seq_sum(a):
    total = np.float32(0)
    for v in a.ravel():
        total = np.float32(total + v)
    return float(total)


def test_vec_input(input):
    return _seq_sum(_vec(input, 1, "input"))


def test_ivec_input(input):
    return int(_ivec(input, 1, "input").sum())


def test_vec2_input(input):
    return _seq_sum(_vec(input, 2, "input"))


def test_vec3_input(input):
    return _seq_sum(_vec(input, 3, "input"))


def test_vec_output():
    return np.full(3, _SWIG_DEFAULT, np.float32)


def test_vec2_output():
    return np.full((3, 3), _SWIG_DEFAULT, np.float32)


def test_vec3_output():
    return np.full((3, 3, 3), _SWIG_DEFAULT, np.float32)


def test_ivec_output():
    return np.full(3, _SWIG_DEFAULT, np.int32)


def test_ivec2_output():
    return np.full((3, 3), _SWIG_DEFAULT, np.int32)


def test_ivec3_output():
    return np.full((3, 3, 3), _SWIG_DEFAULT, np.int32)


def test_vec_argout():
    return 0.0, np.full(10, _SWIG_DEFAULT, np.float32)


def test_vec2_argout():
    return 0.0, np.full((10, 10), _SWIG_DEFAULT, np.float32)


def test_array(v):
    return _vec(v, 1, "v")


def test_not_implemented_exception():
    raise RuntimeError("Not implemented")     # gridpp::not_implemented_exception -> RuntimeError (swig/gridpp.i:21-40)


for _f in (test_vec_input, test_ivec_input, test_vec2_input, test_vec3_input, test_vec_output, test_vec2_output, test_vec3_output, test_ivec_output,
           test_ivec2_output, test_ivec3_output, test_vec_argout, test_vec2_argout, test_array, test_not_implemented_exception):
    _f.__test__ = False       # not pytest tests
