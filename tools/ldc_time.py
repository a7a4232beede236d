"""Time of local_distribution_correction with its fields in HBM: one JSON line per case.

  reference_row   the shape of the reference's own benchmark row (tests/benchmark.py:71): a 200 x 200 grid, 1 000 stations, T = 1,
                  quantiles 0.1 / 0.9, min_points 5 (its structure: Barnes 10 km; grid spacing 1 km, Cartesian)
  nowcast         2000 x 2000 cells at 1 km, 5 000 stations, T = 6, Barnes 10 km, quantiles 0.1 / 0.9, min_points 5

  ms              a host clock around the call (the call ends in a synchronise of the library's stream); torch tensors in, a torch
                  tensor out, so no field crosses PCIe.  Two warm-up calls (they build the station index and size the workspaces),
                  then --reps calls: median, minimum and maximum.
  pairs_*         kept (time, station) pairs per cell: every value of the case is valid and non-negative, so this is T x the
                  number of stations within the localization distance (gridpp.count)

Values are gamma(0.6, 3) rounded to 0.1 mm, a fifth of the stations dry: tied zeros as precipitation has them.

usage: python tools/ldc_time.py [--reps N] [--only NAME,...]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gridpp_amd as gridpp

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--only", default="")
args = ap.parse_args()

CASES = (("reference_row", 200, 1000, 1), ("nowcast", 2000, 5000, 6))

for name, n, S, T in CASES:
    if args.only and name not in args.only.split(","):
        continue
    rng = np.random.default_rng(12)
    lons, lats = np.meshgrid(np.arange(n, dtype=np.float32) * 1000, np.arange(n, dtype=np.float32) * 1000)
    grid = gridpp.Grid(lats, lons, ((),), ((),), gridpp.Cartesian)
    points = gridpp.Points(rng.uniform(0, n * 1000.0, S), rng.uniform(0, n * 1000.0, S), (), (), gridpp.Cartesian)
    st = gridpp.BarnesStructure(10000)
    pobs = np.round(rng.gamma(0.6, 3, (T, S)), 1).astype(np.float32)
    pbg = np.round(rng.gamma(0.6, 3, (T, S)), 1).astype(np.float32)
    pobs[:, rng.random(S) < 0.2] = 0
    bg = torch.from_numpy(np.round(rng.gamma(0.6, 3, (n, n)), 1).astype(np.float32)).cuda()
    pobs, pbg = torch.from_numpy(pobs).cuda(), torch.from_numpy(pbg).cuda()
    if T == 1:
        pobs, pbg = pobs[0], pbg[0]
    pairs = gridpp.count(points, grid, st.localization_distance()) * T

    def call():
        return gridpp.local_distribution_correction(grid, bg, points, pobs, pbg, st, 0.1, 0.9, 5)

    for _ in range(2):
        out = call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    changed = float((out != bg).float().mean())
    print(json.dumps({"case": name, "grid": "%d x %d at 1 km" % (n, n), "stations": S, "times": T, "structure": "Barnes(10000)",
                      "quantiles": [0.1, 0.9], "min_points": 5, "ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3),
                      "ms_max": round(max(ms), 3), "pairs_mean": round(float(pairs.mean()), 1), "pairs_max": int(pairs.max()),
                      "cells_changed": round(changed, 4), "reps": args.reps}), flush=True)
