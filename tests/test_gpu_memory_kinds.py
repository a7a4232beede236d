"""GPU: one call per wrapper family from numpy arrays and from torch tensors on the device, with the same seeded inputs.

Where the input lives, the result lives -- a float32 numpy array for numpy input, a float32 tensor on the input's device for tensor
input -- and the two results agree.  The host path stages the same float32 values through HBM and runs the same kernels, so every
family is held to bit-for-bit equality: downscaling, ensemble downscaling, smart, curve, neighbourhood, window, score, diagnostics,
transform, gamma, local_distribution_correction, gridops and row statistics all gave identical bits before the wrappers were put on
one marshalling layer; no family needed the tolerance of its parity test.

The families that accept GPP_HOST_F64 are called once more with a float64 numpy array of 1024 x 1024 values, the smallest size at
which the wrappers hand float64 over as it is (cast on the device), and must give the bits of the same call on its float32 copy."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def gp():
    import gridpp_amd
    assert gridpp_amd.device_count() > 0
    return gridpp_amd


class Small:
    """8 x 8 fields (E = 3 where a cube is needed) and 16 points"""

    def __init__(self, gp):
        r = np.random.default_rng(20240611)
        lats, lons = np.meshgrid(60 + 0.1 * np.arange(8), 10 + 0.2 * np.arange(8), indexing="ij")
        self.g = gp.Grid(lats, lons, r.uniform(0, 500, (8, 8)), r.uniform(0, 1, (8, 8)))
        olats, olons = np.meshgrid(60.05 + 0.11 * np.arange(5), 10.1 + 0.2 * np.arange(6), indexing="ij")
        self.go = gp.Grid(olats, olons, r.uniform(0, 500, (5, 6)), r.uniform(0, 1, (5, 6)))
        self.p = gp.Points(r.uniform(60, 60.7, 16), r.uniform(10, 11.4, 16), r.uniform(0, 500, 16), r.uniform(0, 1, 16))
        self.st = gp.BarnesStructure(30000, 200)
        self.v, self.v2 = r.normal(0, 1, (8, 8)).astype(F), r.uniform(0, 1, (8, 8)).astype(F)
        self.pos = r.uniform(0.1, 5, (8, 8)).astype(F)
        self.holes = self.v.copy()
        self.holes[2:4, 3:6] = np.nan
        self.c1, self.c2, self.c3 = (r.normal(0, 1, (8, 8, 3)).astype(F) for _ in range(3))
        self.thr = r.normal(0, 0.5, (5, 6)).astype(F)
        self.egrad, self.lgrad = r.normal(-0.0065, 0.001, (8, 8)).astype(F), r.normal(0, 1, (8, 8)).astype(F)
        self.curve_ref, self.curve_fcst = np.sort(r.normal(0, 1, 7)).astype(F), np.sort(r.normal(0, 1, 7)).astype(F)
        self.curves_ref, self.curves_fcst = (np.sort(r.normal(0, 1, (8, 8, 4)), axis=2).astype(F) for _ in range(2))
        self.q = r.uniform(0, 1, (8, 8)).astype(F)
        self.pv, self.pv2 = r.normal(0, 1, 16).astype(F), r.normal(0, 1, 16).astype(F)
        self.ppos, self.ppos2 = r.uniform(0.1, 5, 16).astype(F), r.uniform(0.1, 5, 16).astype(F)
        self.t, self.rh = r.uniform(250, 300, 16).astype(F), r.uniform(0.1, 1, 16).astype(F)
        self.levels = r.uniform(0.01, 0.99, 16).astype(F)
        self.radii = r.uniform(5000, 30000, 16).astype(F)


@pytest.fixture(scope="module")
def k(gp):
    return Small(gp)


# (family, id, call(gp, k, a)): `a` puts a host array where the run wants its fields
CALLS = [
    ("downscaling", "downscaling_bilinear", lambda gp, k, a: gp.downscaling(k.g, k.p, a(k.v), gp.Bilinear)),
    ("downscaling", "nearest", lambda gp, k, a: gp.nearest(k.g, k.go, a(k.c1.transpose(2, 0, 1).copy()))),
    ("downscaling", "simple_gradient", lambda gp, k, a: gp.simple_gradient(k.g, k.p, a(k.v), -0.0065, gp.Nearest)),
    ("downscaling", "full_gradient", lambda gp, k, a: gp.full_gradient(k.g, k.go, a(k.v), a(k.egrad), a(k.lgrad), gp.Bilinear)),
    ("ensemble downscaling", "downscale_probability", lambda gp, k, a: gp.downscale_probability(k.g, k.go, a(k.c1), a(k.thr), gp.Lt)),
    ("ensemble downscaling", "mask_threshold_downscale_consensus",
     lambda gp, k, a: gp.mask_threshold_downscale_consensus(k.g, k.go, a(k.c1), a(k.c2), a(k.c3), a(k.thr), gp.Gt, gp.Mean)),
    ("smart", "smart", lambda gp, k, a: gp.smart(k.g, k.go, a(k.v), 3, k.st)),
    ("curve", "apply_curve", lambda gp, k, a: gp.apply_curve(a(k.v), k.curve_ref, k.curve_fcst, gp.OneToOne, gp.MeanSlope)),
    ("curve", "apply_curve_field", lambda gp, k, a: gp.apply_curve(a(k.v), a(k.curves_ref), a(k.curves_fcst), gp.Zero, gp.NearestSlope)),
    ("curve", "interpolate", lambda gp, k, a: gp.interpolate(a(k.pv), k.curve_fcst, k.curve_ref)),
    ("neighbourhood", "neighbourhood", lambda gp, k, a: gp.neighbourhood(a(k.v), 1, gp.Mean)),
    ("neighbourhood", "neighbourhood_cube", lambda gp, k, a: gp.neighbourhood(a(k.c1), 2, gp.Max)),
    ("neighbourhood", "neighbourhood_brute_force", lambda gp, k, a: gp.neighbourhood_brute_force(a(k.v), 1, gp.Median)),
    ("neighbourhood", "neighbourhood_quantile", lambda gp, k, a: gp.neighbourhood_quantile(a(k.c1), 0.3, 1)),
    ("neighbourhood", "neighbourhood_quantile_fast", lambda gp, k, a: gp.neighbourhood_quantile_fast(a(k.v), 0.5, 1, [-1, 0, 1])),
    ("neighbourhood", "neighbourhood_quantile_fast_field", lambda gp, k, a: gp.neighbourhood_quantile_fast(a(k.v), a(k.q), 1, a(k.curve_ref))),
    ("window", "window", lambda gp, k, a: gp.window(a(k.v), 3, gp.Mean)),
    ("score", "neighbourhood_score", lambda gp, k, a: gp.neighbourhood_score(k.g, k.p, a(k.v), k.pv, 1, gp.Ets, 0.0)),
    ("diagnostics", "wind_speed", lambda gp, k, a: gp.wind_speed(a(k.pv), a(k.pv2))),
    ("diagnostics", "dewpoint", lambda gp, k, a: gp.dewpoint(a(k.t), a(k.rh))),
    ("transform", "log_forward", lambda gp, k, a: gp.Log().forward(a(k.pos))),
    ("transform", "boxcox_backward", lambda gp, k, a: gp.BoxCox(0.5).backward(a(k.c1))),
    ("gamma", "gamma_inv", lambda gp, k, a: gp.gamma_inv(a(k.levels), a(k.ppos), a(k.ppos2))),
    ("gamma", "gamma_forward", lambda gp, k, a: gp.Gamma(2, 1.5).forward(a(k.pos))),
    ("LDC", "local_distribution_correction",
     lambda gp, k, a: gp.local_distribution_correction(k.g, a(k.pos), k.p, a(k.ppos), a(k.ppos2), k.st, 0.1, 0.9)),
    ("gridops", "fill_missing", lambda gp, k, a: gp.fill_missing(a(k.holes))),
    ("gridops", "calc_gradient", lambda gp, k, a: gp.calc_gradient(a(k.pos), a(k.v), gp.LinearRegression, 1)),
    ("gridops", "neighbourhood_search", lambda gp, k, a: gp.neighbourhood_search(a(k.v), a(k.v2), 1, 0.2, 0.8, 0.1)),
    ("gridops", "neighbourhood_search_mask", lambda gp, k, a: gp.neighbourhood_search(a(k.v), a(k.v2), 1, 0.2, 0.8, 0.1, a((k.q > 0.5).astype(np.int32)))),
    ("gridops", "gridding", lambda gp, k, a: gp.gridding(k.g, k.p, a(k.pv), 30000, 1, gp.Mean)),
    ("gridops", "gridding_nearest", lambda gp, k, a: gp.gridding_nearest(k.g, k.p, a(k.pv), 1, gp.Max)),
    ("gridops", "fill", lambda gp, k, a: gp.fill(k.g, a(k.v), k.p, k.radii, -1, False)),
    ("gridops", "doping_circle", lambda gp, k, a: gp.doping_circle(k.g, a(k.v), k.p, a(k.pv), k.radii)),
    ("row statistics", "calc_statistic", lambda gp, k, a: gp.calc_statistic(a(k.v), gp.Median)),
    ("row statistics", "calc_quantile", lambda gp, k, a: gp.calc_quantile(a(k.v), 0.3)),
    ("row statistics", "calc_quantile_cube", lambda gp, k, a: gp.calc_quantile(a(k.c1), a(k.q))),
]


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype == F and np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("family,name,call", CALLS, ids=[c[1] for c in CALLS])
def test_result_lives_where_the_input_lives(gp, k, family, name, call):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    host = call(gp, k, lambda x: x)
    device = call(gp, k, lambda x: torch.from_numpy(x).to(dev))
    assert isinstance(host, np.ndarray) and host.dtype == F
    assert isinstance(device, torch.Tensor) and device.dtype == torch.float32 and device.device == dev
    back = device.cpu().numpy()
    print("%s / %s: %s, max |host - device| = %g" % (family, name, host.shape, np.nanmax(np.abs(host - back), initial=0)))
    assert host.size and np.isfinite(host).any()
    assert same_bits(host, back)


# ---- GPP_HOST_F64: float64 arrays of 2**20 values are handed over as they are ---------------------------------------------------
N = 1024


class Big:
    """one float64 field of 1024 x 1024 values on a grid of that size, and what the calls need beside it"""

    def __init__(self, gp):
        r = np.random.default_rng(77)
        lats, lons = np.meshgrid(50 + 0.01 * np.arange(N), 0.01 * np.arange(N), indexing="ij")
        self.g = gp.Grid(lats, lons, np.zeros((N, N), F), np.zeros((N, N), F))
        olats, olons = np.meshgrid(55 + 0.013 * np.arange(5), 5 + 0.017 * np.arange(6), indexing="ij")
        self.go = gp.Grid(olats, olons, np.zeros((5, 6)), np.zeros((5, 6)))
        self.p = gp.Points(r.uniform(55, 55.1, 16), r.uniform(5, 5.1, 16), np.zeros(16), np.zeros(16))
        self.st = gp.BarnesStructure(2000)
        self.v = r.normal(0, 1, (N, N))
        self.pos = r.uniform(0.1, 5, (N, N))
        self.levels = r.uniform(0.01, 0.99, N * N)
        self.holes = self.v.copy()
        self.holes[100:103, 200:260] = np.nan
        self.thr = r.normal(0, 0.5, (5, 6)).astype(F)
        self.curve_ref, self.curve_fcst = np.sort(r.normal(0, 1, 7)).astype(F), np.sort(r.normal(0, 1, 7)).astype(F)
        self.pv = r.normal(0, 1, 16).astype(F)
        self.ppos, self.ppos2 = r.uniform(0.1, 5, 16), r.uniform(0.1, 5, 16)
        assert self.v.dtype == self.pos.dtype == self.levels.dtype == self.ppos.dtype == np.float64
        assert gp._wants_f64(self.v) and not gp._wants_f64(self.v[:-1])


@pytest.fixture(scope="module")
def b(gp):
    return Big(gp)


# (family, id, call(gp, b, c)): `c` leaves a float64 array as it is or makes its float32 copy
F64_CALLS = [
    ("downscaling", "bilinear", lambda gp, b, c: gp.bilinear(b.g, b.p, c(b.v))),
    ("downscaling", "simple_gradient", lambda gp, b, c: gp.simple_gradient(b.g, b.go, c(b.v), -0.0065, gp.Nearest)),
    ("ensemble downscaling", "downscale_probability", lambda gp, b, c: gp.downscale_probability(b.g, b.go, c(b.v.reshape(N, N, 1)), b.thr, gp.Lt)),
    ("smart", "smart", lambda gp, b, c: gp.smart(b.g, b.go, c(b.v), 3, b.st)),
    ("curve", "apply_curve", lambda gp, b, c: gp.apply_curve(c(b.v), b.curve_ref, b.curve_fcst, gp.OneToOne, gp.MeanSlope)),
    ("neighbourhood", "neighbourhood", lambda gp, b, c: gp.neighbourhood(c(b.v), 1, gp.Mean)),
    ("window", "window", lambda gp, b, c: gp.window(c(b.v), 3, gp.Mean)),
    ("score", "neighbourhood_score", lambda gp, b, c: gp.neighbourhood_score(b.g, b.p, c(b.v), b.pv, 1, gp.Ets, 0.0)),
    ("diagnostics", "wind_speed", lambda gp, b, c: gp.wind_speed(c(b.v.reshape(-1)), c(b.pos.reshape(-1)))),
    ("transform", "log_forward", lambda gp, b, c: gp.Log().forward(c(b.pos))),
    ("gamma", "gamma_inv", lambda gp, b, c: gp.gamma_inv(c(b.levels), c(b.pos.reshape(-1)), c(b.pos.reshape(-1)))),
    ("LDC", "local_distribution_correction",
     lambda gp, b, c: gp.local_distribution_correction(b.g, c(b.pos), b.p, c(b.ppos), c(b.ppos2), b.st, 0.1, 0.9)),
    ("gridops", "fill_missing", lambda gp, b, c: gp.fill_missing(c(b.holes))),
]


@pytest.mark.parametrize("family,name,call", F64_CALLS, ids=[c[1] for c in F64_CALLS])
def test_float64_host_arrays_give_the_bits_of_their_float32_copies(gp, b, family, name, call):
    from64 = call(gp, b, lambda x: x)
    from32 = call(gp, b, lambda x: x.astype(F))
    assert isinstance(from64, np.ndarray) and from64.dtype == F
    print("%s / %s: %s, max |from float64 - from float32| = %g" % (family, name, from64.shape, np.nanmax(np.abs(from64 - from32), initial=0)))
    assert from64.size and np.isfinite(from64).any()
    assert same_bits(from64, from32)
