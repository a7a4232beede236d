"""neighbourhood_score on a device-resident forecast, one JSON line per variant (appended to profiles/score_time.jsonl, or --out):

  workload   4000 x 4000 Geodetic grid on [0, 1] deg^2, 100 000 observations, half width 15, Ets, threshold 0.5, fcst a torch CUDA tensor

  fused         gridpp.neighbourhood_score on the path the library picks (hw 15 <= GPP_SCORE_FUSED_MAXHW: k_score_march)
  general       the same call under GPP_SCORE_GENERAL (k_score_rows + k_score_cols), set through gpp_set_path_override
  composition   what a user had to write before this function existed: gridpp.gridding_nearest (values on the device), the four planes
                in torch, four gridpp.neighbourhood(..., Mean) on device tensors and the Ets arithmetic in torch with the reference's
                promotions.  Its result is compared with `fused` for equality on this input (bit for bit, NaNs in the same places).
  gridding      gridpp.gridding_nearest alone (part of all three): call time minus this is what the classify + box kernels cost

  ms / ms_min   median / best of the repetitions: device events on the library stream (torch runs on that stream here too) around the
                whole call, result allocation and the call's own synchronisation included, after a warm-up
  wall_ms       the same window on the host clock, ending in a device synchronise
  model_bytes   5 per cell: the 1 byte the fused kernel reads and the 4 it writes; model_GBps = model_bytes over (ms - gridding ms), the
                time of everything but the gridding (classification pass included: it moves another 9 bytes per cell)

Fails without a GPU.  usage: python tools/bench_score.py [--reps N] [--size N] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import gridpp_amd as gridpp
from gridpp_amd import _capi

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--size", type=int, default=4000)
ap.add_argument("--obs", type=int, default=100000)
ap.add_argument("--half-width", type=int, default=15)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_time.jsonl"))
args = ap.parse_args()

if not torch.cuda.is_available() or gridpp.device_count() == 0:
    sys.exit("bench_score.py: no GPU visible -- a time measured anywhere else says nothing about this path")
if gridpp.active_overrides():
    sys.exit("bench_score.py: path overrides are set: %s" % gridpp.active_overrides())

N, S, HW, TH = args.size, args.obs, args.half_width, 0.5
rng = np.random.default_rng(2026)
lats, lons = np.meshgrid(np.linspace(0, 1, N), np.linspace(0, 1, N), indexing="ij")
grid = gridpp.Grid(lats, lons)
points = gridpp.Points(rng.random(S), rng.random(S))
ref = rng.random(S).astype(np.float32)
handle = C.c_void_p()
assert _capi.lib().gpp_get_stream(C.byref(handle)) == _capi.GPP_OK
stream = torch.cuda.ExternalStream(handle.value)


def ets(a, b, c, d):
    """metric_optimizer.cpp:208-214 in torch, the reference's promotions"""
    n = a + b + c + d
    ar = ((a + b).double() / n.double() * (a + c).double()).float()
    den = a + b + c - ar
    value = ((a - ar).double() / den.double()).float()
    return torch.where(den == 0, torch.full_like(value, float("nan")), value)


with torch.cuda.stream(stream):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    fcst = torch.rand((N, N), device="cuda", generator=gen)
    dref = torch.from_numpy(ref).cuda()

    def fused():
        return gridpp.neighbourhood_score(grid, points, fcst, ref, HW, gridpp.Ets, TH)

    def general():
        _capi.lib().gpp_set_path_override(b"GPP_SCORE_GENERAL", b"1")
        try:
            return gridpp.neighbourhood_score(grid, points, fcst, ref, HW, gridpp.Ets, TH)
        finally:
            _capi.lib().gpp_set_path_override(b"GPP_SCORE_GENERAL", None)

    def gridding():
        return gridpp.gridding_nearest(grid, points, dref, 1, gridpp.Mean)

    def composition():
        ref_grid = gridding()
        ok = torch.isfinite(ref_grid) & torch.isfinite(fcst)
        hit, above = fcst > TH, ref_grid > TH
        below = ref_grid <= TH
        hoods = [gridpp.neighbourhood((ok & m).float(), HW, gridpp.Mean) for m in (hit & above, hit & below, ~hit & above, ~hit & below)]
        return ets(*hoods)

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record(stream)
        f()
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3

    variants = (("fused", fused), ("general", general), ("composition", composition), ("gridding", gridding))
    results = {}
    for name, f in variants:            # warm-up, and the results that are compared
        for _ in range(3):
            results[name] = f()
    torch.cuda.synchronize()

    def same(x, y):
        return bool(torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(y, nan=7.0)))

    equal_general, equal_composition = same(results["fused"], results["general"]), same(results["fused"], results["composition"])
    nan_share = float(torch.isnan(results["fused"]).float().mean())
    results.clear()
    times = {name: [] for name, _ in variants}
    for _ in range(args.reps):          # alternated: drift and other people's work hit all variants alike
        for name, f in variants:
            times[name].append(timed(f))

cells = N * N
grid_ms = float(np.median([t[0] for t in times["gridding"]]))
lines = []
for name, _ in variants:
    ev, wall = [t[0] for t in times[name]], [t[1] for t in times[name]]
    line = {"case": name, "grid": [N, N], "observations": S, "half_width": HW, "metric": "Ets", "reps": args.reps, "ms": round(float(np.median(ev)), 3),
            "ms_min": round(min(ev), 3), "ms_max": round(max(ev), 3), "wall_ms": round(float(np.median(wall)), 3)}
    if name in ("fused", "general"):
        rest = float(np.median(ev)) - grid_ms
        line.update({"ms_without_gridding": round(rest, 3), "model_bytes": 5 * cells, "model_GBps": round(5 * cells / (rest / 1e3) / 1e9, 1)})
    if name == "general":
        line["equal_to_fused"] = equal_general
    if name == "composition":
        line["equal_to_fused"] = equal_composition
    if name == "fused":
        line["nan_share_of_result"] = round(nan_share, 4)
    print(json.dumps(line), flush=True)
    lines.append(line)
with open(args.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
if not equal_general:
    sys.exit("bench_score.py: the two paths of the library do not agree")
