"""corr(p1, many) on the GPU: the list form of 2000 points against the loop of scalar calls it replaces, and the handle
form on a 4000 x 4000 grid with a host and with a device result.  Each figure is the median (min, max) of 5 calls after a warm-up call,
timed on the host around calls that end in a stream synchronise.

    python tools/bench_structure_corr.py
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gridpp_amd as gridpp   # noqa: E402


def median5(f):
    f()
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts), min(ts), max(ts)


rng = np.random.default_rng(5)
s = gridpp.BarnesStructure(10000, 200, 0.5)
p1 = gridpp.Point(60, 10, 100, 0.5)
pts = [gridpp.Point(60 + rng.uniform(-0.3, 0.3), 10 + rng.uniform(-0.6, 0.6), rng.uniform(0, 300), rng.uniform(0, 1)) for _ in range(2000)]
loop = median5(lambda: np.array([s._corr(p1, q, 0) for q in pts], np.float32))
one = median5(lambda: s.corr(p1, pts))
a = np.array([s._corr(p1, q, 0) for q in pts], np.float32)
b = s.corr(p1, pts)
print("list form, 2000 points: loop of scalar calls %.3f ms (min %.3f max %.3f); one call %.3f ms (min %.3f max %.3f); equal bits: %s"
      % (loop[0] * 1e3, loop[1] * 1e3, loop[2] * 1e3, one[0] * 1e3, one[1] * 1e3, one[2] * 1e3, np.array_equal(a.view(np.uint32), b.view(np.uint32))), flush=True)

Y = X = 4000
lats, lons = np.meshgrid(np.linspace(50, 70, Y), np.linspace(0, 30, X), indexing="ij")
elevs = rng.uniform(0, 300, (Y, X)).astype(np.float32)
lafs = rng.uniform(0, 1, (Y, X)).astype(np.float32)
grid = gridpp.Grid(lats, lons, elevs, lafs)
n = Y * X
host = median5(lambda: s.corr(p1, grid))
dev = median5(lambda: s.corr(p1, grid, device="cuda"))
h, d = s.corr(p1, grid), s.corr(p1, grid, device="cuda").cpu().numpy()
# The kernel reads x, y, z of a point, and its elevation and land-area fraction only in a wave where some lane passed the localization cut
# (DESIGN.md 4.4): 12 B + 4 B per point where every wave is cut off, 20 B + 4 B where none is.  Rates are bytes over the whole call.
lo, hi = 16 * n, 24 * n


def rate(t):
    return "%.0f - %.0f GB/s for %d - %d MB (%.0f - %.0f %% of the 6.29 TB/s measured peak)" % (lo / t / 1e9, hi / t / 1e9, lo / 1e6, hi / 1e6,
                                                                                                100 * lo / t / 6.29e12, 100 * hi / t / 6.29e12)


print("handle form, %d x %d grid: host result %.3f ms (min %.3f max %.3f); device result %.3f ms (min %.3f max %.3f); equal: %s; %d of %d values nonzero"
      % (Y, X, host[0] * 1e3, host[1] * 1e3, host[2] * 1e3, dev[0] * 1e3, dev[1] * 1e3, dev[2] * 1e3, np.array_equal(h, d), np.count_nonzero(h), n), flush=True)
print("  device-result call: " + rate(dev[0]), flush=True)
for name, st in (("soar", gridpp.SoarStructure(10000, 200, 0.5)), ("powerlaw", gridpp.PowerlawStructure(10000, 200, 0.5)),
                 ("cressman", gridpp.CressmanStructure(10000, 200, 0.5))):
    t = median5(lambda: st.corr(p1, grid, device="cuda"))
    print("  %s, device result %.3f ms: %s" % (name, t[0] * 1e3, rate(t[0])), flush=True)
# no correlation cut off: a localization distance that covers the grid (every wave reads all five arrays, every lane runs all three factors)
wide = gridpp.BarnesStructure(2000000, 200, 0.5)
t = median5(lambda: wide.corr(p1, grid, device="cuda"))
print("  barnes h = 2000 km (no point cut off), device result %.3f ms: %.0f GB/s for %d MB" % (t[0] * 1e3, hi / t[0] / 1e9, hi / 1e6), flush=True)
