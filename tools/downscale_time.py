"""simple_gradient / full_gradient, 1000 x 1000 grid -> 4000 x 4000 grid, Nearest / Bilinear, T = 1 and 24: one JSON line per case.

  fused_ms     the library call on torch tensors (device path), hipEvents on the torch stream around warmed calls, median
               (fused_min_ms / fused_max_ms: the extremes of the timed samples; their difference is the spread of the measurement)
  composed_ms  the same result composed as the reference builds it (src/api/gradient.cpp:26-81): the existing nearest / bilinear on
               the stacked fields (values, gradients, elevations, lafs; T (1 or 3) + 2 levels), then a torch elementwise pass --
               measured in the same process, alternated with the fused call (the stacking itself is not timed)
  bytes        from shapes: the fields read once (T levels of each input field, the input elevations / lafs, the output
               elevations / lafs) and the result written once -- what a single pass has to move; GB/s and the share of the
               8.0 TB/s peak follow from the fused time
  host_ms      numpy in -> numpy out (float32 inputs, the result back in host memory), median

usage: python tools/downscale_time.py [--reps N] [--host-reps N] [--only full_bilinear_24]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gridpp_amd as gridpp

PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--only", default="")
args = ap.parse_args()

rng = np.random.default_rng(42)
NI, NO = 1000, 4000
ilats, ilons = np.meshgrid(np.linspace(59, 61, NI), np.linspace(9, 12, NI), indexing="ij")
olats, olons = np.meshgrid(np.linspace(59, 61, NO, dtype=np.float32), np.linspace(9, 12, NO, dtype=np.float32), indexing="ij")
ielevs, ilafs = rng.uniform(0, 1500, (NI, NI)).astype(np.float32), rng.uniform(0, 1, (NI, NI)).astype(np.float32)
oelevs, olafs = rng.uniform(0, 1500, (NO, NO)).astype(np.float32), rng.uniform(0, 1, (NO, NO)).astype(np.float32)
igrid = gridpp.Grid(ilats, ilons, ielevs, ilafs)
ogrid = gridpp.Grid(olats, olons, oelevs, olafs)
d_ielev, d_ilaf = torch.from_numpy(ielevs).cuda(), torch.from_numpy(ilafs).cuda()
d_oelev, d_olaf = torch.from_numpy(oelevs).cuda(), torch.from_numpy(olafs).cuda()


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def composed_full(ds, v, eg, lg):
    T = v.shape[0]
    stacked = torch.cat([v, eg, d_ielev[None], lg, d_ilaf[None]])

    def run():
        d = gridpp.bilinear(igrid, ogrid, stacked) if ds == gridpp.Bilinear else gridpp.nearest(igrid, ogrid, stacked)
        dv, deg, de, dlg, dl = d[:T], d[T:2 * T], d[2 * T], d[2 * T + 1:3 * T + 1], d[3 * T + 1]
        lok = torch.isfinite(d_olaf) & torch.isfinite(dl)
        eok = torch.isfinite(d_oelev) & torch.isfinite(de)
        laf_corr = torch.where(lok, dlg * (d_olaf - dl), torch.zeros((), device="cuda"))
        elev_corr = torch.where(eok, deg * (d_oelev - de), torch.zeros((), device="cuda"))
        return dv + (laf_corr + elev_corr)
    return run


def composed_simple(ds, v, g):
    T = v.shape[0]
    stacked = torch.cat([v, d_ielev[None]])

    def run():
        d = gridpp.bilinear(igrid, ogrid, stacked) if ds == gridpp.Bilinear else gridpp.nearest(igrid, ogrid, stacked)
        return d[:T] + (d_oelev - d[T]) * g
    return run


for fn in ("simple", "full"):
    for ds, dsname in ((gridpp.Nearest, "nearest"), (gridpp.Bilinear, "bilinear")):
        for T in (1, 24):
            name = "%s_%s_%d" % (fn, dsname, T)
            if args.only and name not in args.only.split(","):
                continue
            v = torch.randn((T, NI, NI), device="cuda")
            if fn == "full":
                eg = -0.0065 + 0.002 * torch.randn((T, NI, NI), device="cuda")
                lg = 2 + torch.randn((T, NI, NI), device="cuda")
                fused = lambda: gridpp.full_gradient(igrid, ogrid, v, eg, lg, ds)   # noqa: E731
                comp = composed_full(ds, v, eg, lg)
                nbytes = 4 * (3 * T * NI * NI + 2 * NI * NI + 2 * NO * NO + T * NO * NO)
                host_in = [a.cpu().numpy() for a in (v, eg, lg)]
                host = lambda: gridpp.full_gradient(igrid, ogrid, *host_in, ds)   # noqa: E731
            else:
                fused = lambda: gridpp.simple_gradient(igrid, ogrid, v, -0.0065, ds)   # noqa: E731
                comp = composed_simple(ds, v, -0.0065)
                nbytes = 4 * (T * NI * NI + NI * NI + NO * NO + T * NO * NO)
                hv = v.cpu().numpy()
                host = lambda: gridpp.simple_gradient(igrid, ogrid, hv, -0.0065, ds)   # noqa: E731
            # the two paths agree (Nearest and Bilinear run the same float expressions)
            same = bool(torch.equal(torch.nan_to_num(fused().reshape(T, -1)), torch.nan_to_num(comp().reshape(T, -1))))
            fused(); comp()
            tf, tc = [], []
            for _ in range(args.reps):
                tf.append(timed(fused))
                tc.append(timed(comp))
            torch.cuda.empty_cache()
            host()
            import time
            th = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                host()
                th.append((time.perf_counter() - t0) * 1e3)
            f_ms = float(np.median(tf))
            print(json.dumps({"case": name, "grid": "%d^2 -> %d^2" % (NI, NO), "T": T, "fused_ms": round(f_ms, 3),
                              "fused_min_ms": round(min(tf), 3), "fused_max_ms": round(max(tf), 3),
                              "composed_ms": round(float(np.median(tc)), 3), "speedup": round(float(np.median(tc)) / f_ms, 2),
                              "bytes": nbytes, "GBps": round(nbytes / f_ms / 1e6, 1), "share_of_8TBps": round(nbytes / PEAK / (f_ms / 1e3), 3),
                              "host_ms": round(float(np.median(th)), 2), "bit_equal_to_composed": same, "reps": args.reps}), flush=True)
            del v
            torch.cuda.empty_cache()
