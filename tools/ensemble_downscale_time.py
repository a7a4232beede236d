"""downscale_probability / mask_threshold_downscale_consensus (Mean, Median), E = 50, 1000^2 -> 4000^2 and 4000^2 -> 4000^2, and one
timing of smart: one JSON line per case.

  fused_ms        the library call on torch tensors (device path), hipEvents on the torch stream around warmed calls, median
                  (fused_min_ms / fused_max_ms: the extremes of the timed samples; their difference is the spread of the measurement)
  composed_ms     the same product composed from what the library had before these entry points: `nearest` of the field
                  arange(Y X) for the index (exact below 2^24 cells), then gather + compare + reduce in torch -- measured in the
                  same process, alternated with the fused call.  The composed Mean sums in torch's order and the composed Median is
                  torch.nanmedian (lower middle element), so the composed results are close to, not bit-equal to, the fused ones.
  distinct_bytes  distinct input cells touched x 4 E x cubes read + output cells x (4 threshold + 4 out + 4 + 4 index written and
                  read back); requested_bytes counts every output cell's member reads instead (upsampling repeats them; the repeats
                  come from the caches).  share_* = bytes / 8.0 TB/s / fused time.

usage: python tools/ensemble_downscale_time.py [--reps N] [--only NAME,...] [--smart]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gridpp_amd as gridpp

PEAK = 8.0e12
E = 50

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--only", default="")
ap.add_argument("--smart", action="store_true")
args = ap.parse_args()


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def grid(n, dtype=np.float32):
    lats, lons = np.meshgrid(np.linspace(59, 61, n, dtype=dtype), np.linspace(9, 12, n, dtype=dtype), indexing="ij")
    return gridpp.Grid(lats, lons)


NO = 4000
ogrid = grid(NO)
thr = torch.randn((NO, NO), device="cuda")
t = thr.reshape(-1, 1)
nan = torch.full((), float("nan"), device="cuda")

for NI in (1000, 4000):
    igrid = ogrid if NI == NO else grid(NI)
    cubes = [torch.randn((NI, NI, E), device="cuda") for _ in range(3)]
    for c in cubes:
        c[torch.rand((NI, NI, E), device="cuda") < 0.02] = float("nan")
    vt, vf, tv = cubes
    iota = torch.arange(NI * NI, device="cuda", dtype=torch.float32).reshape(NI, NI)

    def index():
        return gridpp.nearest(igrid, ogrid, iota).reshape(-1).to(torch.int64)

    def comp_probability():
        v = tv.view(-1, E)[index()]
        ok = torch.isfinite(v)
        return ((v <= t) & ok).sum(1).float() / ok.sum(1).float()

    def masked():
        idx = index()
        g = tv.view(-1, E)[idx]
        m = torch.where(g <= t, vt.view(-1, E)[idx], vf.view(-1, E)[idx])
        return torch.where(torch.isfinite(g), m, nan)

    def comp_mean():
        m = masked()
        ok = torch.isfinite(m)
        return torch.where(ok, m, torch.zeros((), device="cuda")).sum(1) / ok.sum(1).float()

    def comp_median():
        return torch.nanmedian(masked(), dim=1).values

    distinct = int(torch.unique(index()).numel())
    rows = (("probability", 1, lambda: gridpp.downscale_probability(igrid, ogrid, tv, thr, gridpp.Leq), comp_probability),
            ("mask_mean", 3, lambda: gridpp.mask_threshold_downscale_consensus(igrid, ogrid, vt, vf, tv, thr, gridpp.Leq, gridpp.Mean), comp_mean),
            ("mask_median", 3, lambda: gridpp.mask_threshold_downscale_consensus(igrid, ogrid, vt, vf, tv, thr, gridpp.Leq, gridpp.Median), comp_median))
    for name, ncubes, fused, comp in rows:
        case = "%s_%d" % (name, NI)
        if args.only and case not in args.only.split(","):
            continue
        a, b = fused().reshape(-1), comp()
        close = float((torch.nan_to_num(a - b).abs() <= 1e-5 * (1 + torch.nan_to_num(b).abs())).float().mean())
        del a, b
        tf, tc = [], []
        for _ in range(args.reps):
            tf.append(timed(fused))
            tc.append(timed(comp))
        torch.cuda.empty_cache()
        f_ms, c_ms = float(np.median(tf)), float(np.median(tc))
        dbytes = distinct * 4 * E * ncubes + NO * NO * 16
        rbytes = NO * NO * 4 * E * ncubes + NO * NO * 16
        print(json.dumps({"case": case, "grid": "%d^2 x %d -> %d^2" % (NI, E, NO), "fused_ms": round(f_ms, 3), "composed_ms": round(c_ms, 3),
                          "fused_min_ms": round(min(tf), 3), "fused_max_ms": round(max(tf), 3),
                          "speedup": round(c_ms / f_ms, 2), "distinct_cells": distinct, "distinct_bytes": dbytes, "requested_bytes": rbytes,
                          "share_of_8TBps_distinct": round(dbytes / PEAK / (f_ms / 1e3), 3),
                          "share_of_8TBps_requested": round(rbytes / PEAK / (f_ms / 1e3), 3),
                          "cells_within_1e-5_of_composed": round(close, 4), "reps": args.reps}), flush=True)
    del cubes, vt, vf, tv
    torch.cuda.empty_cache()

if args.smart:
    # 1000^2 -> 2000^2 over 10 x 10 degrees (input spacing about 1.1 km north-south), terrain on both grids, Barnes(5000, 200), num 10
    rng = np.random.default_rng(3)

    def terrain(n):
        lats, lons = np.meshgrid(np.linspace(55, 65, n, dtype=np.float32), np.linspace(5, 15, n, dtype=np.float32), indexing="ij")
        elev = 400 + 300 * np.sin(lats * 7) * np.cos(lons * 5) + rng.uniform(0, 100, lats.shape)
        return gridpp.Grid(lats, lons, elev.astype(np.float32))
    ig, og = terrain(1000), terrain(2000)
    v = torch.randn((1000, 1000), device="cuda")
    st = gridpp.BarnesStructure(5000, 200)
    gridpp.smart(ig, og, v, 10, st)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gridpp.smart(ig, og, v, 10, st)
    torch.cuda.synchronize()
    print(json.dumps({"case": "smart", "grid": "1000^2 -> 2000^2, 10 x 10 degrees", "structure": "Barnes(5000, 200)", "num": 10,
                      "ms": round((time.perf_counter() - t0) * 1e3, 1), "reps": 1}), flush=True)
