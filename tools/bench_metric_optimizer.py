"""get_optimal_threshold and metric_optimizer_curve on one MI355X, device-resident, one JSON line per case (printed, and appended to
profiles/metric_optimizer_time.txt or --out):

  get_optimal_threshold   the reference benchmark's case (tests/benchmark.py:83 there): two randn vectors of 10^6 values, threshold 0, Ets
  metric_optimizer_curve  20 thresholds, linspace(-1.5, 1.5, 20), on the same vectors: one sort, the thresholds swept four to a workgroup
  calc_score              today's counting pass on the same vectors (threshold 0, fthreshold 0, Ets): the yardstick.  The sweep does a
                          sort and a scan on top of a counting pass, so a small multiple of this time is what the two above are read
                          against.

Every case is warmed up first; then device events bracket a window of whole calls that lasts at least --window seconds (0.5), and the
time per call is the window over its calls.  Every call ends in the library's own synchronisation, so the window holds launch, copy-back
and host time as a caller sees them.

Fails without a GPU.  usage: python tools/bench_metric_optimizer.py [--window S] [--n N] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import gridpp_amd as gridpp

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metric_optimizer_time.txt"))
args = ap.parse_args()

if not torch.cuda.is_available() or gridpp.device_count() == 0:
    sys.exit("bench_metric_optimizer.py: no GPU visible -- a time measured anywhere else says nothing about this path")
if gridpp.active_overrides():
    sys.exit("bench_metric_optimizer.py: path overrides are set: %s" % gridpp.active_overrides())


def window(f):
    """-> (ms per call, calls): calls doubled until the bracketed window lasts args.window seconds"""
    calls = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            f()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= args.window * 1e3:
            return ms / calls, calls
        calls = max(calls * 2, int(calls * args.window * 1e3 / max(ms, 1e-3) * 1.1) + 1)


rng = np.random.default_rng(20240614)
ref, fcst = rng.standard_normal(args.n).astype(np.float32), rng.standard_normal(args.n).astype(np.float32)
d_ref, d_fcst = torch.from_numpy(ref).cuda(), torch.from_numpy(fcst).cuda()
thresholds = np.linspace(-1.5, 1.5, 20).astype(np.float32)

cases = [
    ("calc_score, threshold 0, Ets, device-resident", 1, lambda: gridpp.calc_score(d_ref, d_fcst, 0.0, 0.0, gridpp.Ets)),
    ("get_optimal_threshold, threshold 0, Ets, device-resident", 1, lambda: gridpp.get_optimal_threshold(d_ref, d_fcst, 0.0, gridpp.Ets)),
    ("metric_optimizer_curve, 20 thresholds, Ets, device-resident", 20, lambda: gridpp.metric_optimizer_curve(d_ref, d_fcst, thresholds, gridpp.Ets)),
]

lines = []
for name, T, call in cases:
    for _ in range(2):   # warm-up of this shape: the workspaces
        result = call()
    ms, calls = window(call)
    line = {"case": name, "values": args.n, "thresholds": T, "ms_per_call": round(ms, 4), "ms_per_threshold": round(ms / T, 4), "calls_in_window": calls,
            "window_ms": round(ms * calls, 1)}
    if T == 1:
        line["result"] = float(result)
    else:
        line["valid_thresholds"] = int(len(result[0]))
    print(json.dumps(line), flush=True)
    lines.append(line)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    f.write("# python tools/bench_metric_optimizer.py --window %g --n %d\n" % (args.window, args.n))
    for line in lines:
        f.write(json.dumps(line) + "\n")
