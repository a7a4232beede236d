"""The headline OI call behind a FRESH Points object: what one analysis costs when nothing of the observation set is remembered -- the Points
constructor, the observation index, the pair table (csrc/oi_pair_table.h: built by the first call that needs it) and the call itself, from
the constructor to the synchronised result.  The Grid, the fields and the library's workspaces are warm (one call with another Points
first).  For A/B runs of two libraries (GPP_LIB), alternated run by run.  usage: oi_fresh_points.py [samples] [ny] [obs] [max_points]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import gridpp_amd as gridpp
from tools.bench_cases import make_workload
n = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ny = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
S = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
mp = int(sys.argv[4]) if len(sys.argv) > 4 else 30
lats, lons, bg, plat, plon, obs, ratios, pbg = make_workload(ny, ny, S, 1002, 0, ny)
grid, st = gridpp.Grid(lats, lons), gridpp.BarnesStructure(10000)
d = [torch.from_numpy(a).cuda() for a in (bg, obs, ratios, pbg)]
warm = gridpp.Points(plat[::-1].copy(), plon[::-1].copy())
for _ in range(2):
    gridpp.optimal_interpolation(grid, d[0], warm, d[1], d[2], d[3], st, mp)
torch.cuda.synchronize()
ms, build, steady = [], [], []
for _ in range(n):
    t0 = time.perf_counter()
    points = gridpp.Points(plat, plon)
    gridpp.optimal_interpolation(grid, d[0], points, d[1], d[2], d[3], st, mp)
    torch.cuda.synchronize()
    ms.append((time.perf_counter() - t0) * 1e3)
    build.append(gridpp.oi_last_stats().get("pair_table_build_ms", 0.0))
    t0 = time.perf_counter()
    gridpp.optimal_interpolation(grid, d[0], points, d[1], d[2], d[3], st, mp)
    torch.cuda.synchronize()
    steady.append((time.perf_counter() - t0) * 1e3)
print("fresh Points + one analysis: median %.3f ms (%s); pair_table_build_ms median %.3f; the same Points once more: median %.3f ms (%dx%d, %d obs, mp %d)"
      % (np.median(ms), " ".join("%.3f" % v for v in ms), np.median(build), np.median(steady), ny, ny, S, mp))
