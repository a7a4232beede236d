"""gamma_inv and the Gamma transform on one MI355X, one JSON line per case (printed, and appended to profiles/gamma_time.txt or --out):

  gamma_inv, device-resident   the reference benchmark's case (tests/benchmark.py:78 there: 5 x 201 x 476 = 478 380 values, levels
                               0.05 + 0.9 U, shape and scale U(0, 1)) and 16 M values of the wide domain (shape log-uniform in
                               [1e-2, 1e3], scale in [1e-3, 1e3], levels U(0, 1))
  Gamma(1, 2, 0.01), device    forward on a 4000 x 4000 field that is 60 % zeros, the rest gamma-distributed; backward on its result
  the same from numpy arrays   gamma_inv (reference case) and forward / backward (4000 x 4000), numpy in, numpy out: staging included

Every case is warmed up first; then device events bracket a window of whole calls that lasts at least --window seconds (0.5), and the
time per call is the window over its calls.  bytes: 4 bytes per input and output value.  The arithmetic per value is not in this file:
tools/gamma_trip_counts.cpp counts the series terms, fraction steps and inverse steps of the same source on the same inputs
(--dump-inputs FILE writes the first 2^20 values of every case for it).

Fails without a GPU.  usage: python tools/bench_gamma.py [--window S] [--out FILE] [--dump-inputs FILE]"""
import argparse
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import gridpp_amd as gridpp

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gamma_time.txt"))
ap.add_argument("--dump-inputs", default="")
ap.add_argument("--side", type=int, default=4000)
args = ap.parse_args()

if not torch.cuda.is_available() or gridpp.device_count() == 0:
    sys.exit("bench_gamma.py: no GPU visible -- a time measured anywhere else says nothing about this path")

F = np.float32
rng = np.random.default_rng(20240614)


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


def log_uniform(lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(F)


def reference_case():
    n = 5 * 201 * 476
    return (0.05 + 0.9 * rng.random(n)).astype(F), np.maximum(rng.random(n), 1e-7).astype(F), np.maximum(rng.random(n), 1e-7).astype(F)


def wide_case(n):
    return rng.random(n).astype(F), log_uniform(1e-2, 1e3, n), log_uniform(1e-3, 1e3, n)


def precipitation(n):
    field = rng.gamma(1.0, 2.0, n).astype(F)
    field[rng.random(n) < 0.6] = 0
    return field


def dev(a):
    return torch.from_numpy(a).cuda()


PARAMS = (1.0, 2.0, 0.01)
gamma = gridpp.Gamma(*PARAMS)
N = args.side * args.side
ref, wide, field = reference_case(), wide_case(1 << 24), precipitation(N)
d_ref, d_wide, d_field = [dev(a) for a in ref], [dev(a) for a in wide], dev(field)
d_normal = gamma.forward(d_field)
normal = d_normal.cpu().numpy()
assert np.isfinite(normal).all()

cases = [
    ("gamma_inv reference-benchmark case, device-resident", 0, ref, lambda: gridpp.gamma_inv(*d_ref), 4),
    ("gamma_inv wide domain 16 M, device-resident", 0, wide, lambda: gridpp.gamma_inv(*d_wide), 4),
    ("Gamma(1, 2, 0.01).forward %d x %d, device-resident" % (args.side, args.side), 1, (field,), lambda: gamma.forward(d_field), 2),
    ("Gamma(1, 2, 0.01).backward %d x %d, device-resident" % (args.side, args.side), 2, (normal,), lambda: gamma.backward(d_normal), 2),
    ("gamma_inv reference-benchmark case, numpy to numpy", 0, ref, lambda: gridpp.gamma_inv(*ref), 4),
    ("Gamma(1, 2, 0.01).forward %d x %d, numpy to numpy" % (args.side, args.side), 1, (field,), lambda: gamma.forward(field), 2),
    ("Gamma(1, 2, 0.01).backward %d x %d, numpy to numpy" % (args.side, args.side), 2, (normal,), lambda: gamma.backward(normal), 2),
]

if args.dump_inputs:
    with open(args.dump_inputs, "wb") as f:
        for name, kind, arrays, _, _ in cases[:4]:
            n = min(len(arrays[0]), 1 << 20)
            f.write(struct.pack("<ii3f", kind, n, *PARAMS))
            for a in arrays:
                f.write(np.ascontiguousarray(a[:n], F).tobytes())

lines = []
for name, kind, arrays, call, words in cases:
    n = len(arrays[0])
    for _ in range(2):   # warm-up of this shape: workspaces, staging and pinned result buffers
        out = call()
    del out
    ms, calls = window(call)
    line = {"case": name, "values": n, "ms_per_call": round(ms, 4), "values_per_s": round(n / (ms / 1e3), 1), "calls_in_window": calls,
            "window_ms": round(ms * calls, 1), "bytes": 4 * words * n, "gbps": round(4 * words * n / (ms / 1e3) / 1e9, 2)}
    print(json.dumps(line), flush=True)
    lines.append(line)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    f.write("# python tools/bench_gamma.py --window %g --side %d\n" % (args.window, args.side))
    for line in lines:
        f.write(json.dumps(line) + "\n")
