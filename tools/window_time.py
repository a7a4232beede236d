"""window on device-resident tensors, one JSON line per (matrix, call) (appended to profiles/window_time.jsonl, or --out):

  matrices   4M x 66 (a 2000 x 2000 grid, 66 lead times) and 16M x 24 (a 4000 x 4000 grid, 24 hours)
  calls      sum_3 (centred), sum_24_before, mean_6_before, max_7, median_5 on the path the library picks (all fit the fused tile), and
             sum_24_before_general: the same Sum with the general path forced (GPP_WINDOW_GENERAL, set through gpp_set_path_override)

  ms            the library call (gridpp.window on a torch CUDA tensor, result allocation included), device events around a synchronised
                window, warmed up; median, minimum and maximum of the repetitions
  copy_ms       NOT the code under test: a device-to-device copy of the same number of bytes (out.copy_(in): one read and one write of
                the matrix, which is what the fused kernels need), measured in the same process, alternated with the call
  copy_over_ms  copy_ms / ms: the share of the copy's rate the call reaches (1.0 = as fast as moving the matrix once)
  bytes         8 per value: what the algorithm needs from the shapes (the general Sum moves 24: it writes and reads two planes)

Fails without a GPU.  usage: python tools/window_time.py [--reps N] [--only NAME,...] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import gridpp_amd as gridpp
from gridpp_amd import _capi

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--only", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_time.jsonl"))
args = ap.parse_args()

if not torch.cuda.is_available() or gridpp.device_count() == 0:
    sys.exit("window_time.py: no GPU visible -- a time measured anywhere else says nothing about this path")


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


MATRICES = (("4Mx66", 4000000, 66), ("16Mx24", 16000000, 24))
# name, length, statistic, before, general path forced
CALLS = (("sum_3", 3, gridpp.Sum, False, False), ("sum_24_before", 24, gridpp.Sum, True, False), ("mean_6_before", 6, gridpp.Mean, True, False),
         ("max_7", 7, gridpp.Max, False, False), ("median_5", 5, gridpp.Median, False, False), ("sum_24_before_general", 24, gridpp.Sum, True, True))

lines = []
for mname, Y, T in MATRICES:
    gen = torch.Generator(device="cuda")
    gen.manual_seed(Y + T)
    x = torch.rand((Y, T), device="cuda", generator=gen) * 4   # hourly-precipitation-like magnitudes
    x[torch.rand((Y, T), device="cuda", generator=gen) < 0.01] = float("nan")
    spare = torch.empty_like(x)

    def copy():
        spare.copy_(x)

    for cname, length, statistic, before, general in CALLS:
        case = mname + "_" + cname
        if args.only and case not in args.only.split(","):
            continue

        def call():
            return gridpp.window(x, length, statistic, before)

        if general:
            _capi.lib().gpp_set_path_override(b"GPP_WINDOW_GENERAL", b"1")
        try:
            for _ in range(3):
                call()
                copy()
            tw, tc = [], []
            for _ in range(args.reps):
                tw.append(timed(call))
                tc.append(timed(copy))
        finally:
            _capi.lib().gpp_set_path_override(b"GPP_WINDOW_GENERAL", None)
        w_ms, c_ms = float(np.median(tw)), float(np.median(tc))
        line = {"case": case, "shape": [Y, T], "length": length, "statistic": int(statistic), "before": before, "general_path_forced": general,
                "ms": round(w_ms, 3), "ms_min": round(min(tw), 3), "ms_max": round(max(tw), 3), "copy_ms": round(c_ms, 3), "copy_ms_min": round(min(tc), 3),
                "copy_ms_max": round(max(tc), 3), "copy_over_ms": round(c_ms / w_ms, 3), "bytes": 8 * Y * T,
                "GBps_of_8_bytes_per_value": round(8 * Y * T / (w_ms / 1e3) / 1e9, 1), "copy_GBps": round(8 * Y * T / (c_ms / 1e3) / 1e9, 1), "reps": args.reps}
        print(json.dumps(line), flush=True)
        lines.append(line)
    del x, spare
    torch.cuda.empty_cache()
    _capi.lib().gpp_release_workspaces()

with open(args.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
