"""gpp_neighbourhood_quantiles_fast and gpp_neighbourhood_cdf on device-resident cubes, one JSON line per (case, number of levels),
appended to profiles/nbh_quantiles_time.jsonl (or --out).  The library is called through ctypes.

  cases      config4 (4000 x 4000 x 100) and tile (530 x 4000 x 100, a rank's row tile), halfwidth 15, 11 thresholds 0 .. 10 over uniform
             [0, 10) members, with 1, 3, 5 and 9 levels evenly spaced inside (0, 1) (an odd count holds 0.5, the level ON a threshold's
             expected rank), plus the cdf

  ms                     one many-level (or cdf) call, device events around a synchronised window, 3 warm-up calls, the median of 7 (--reps);
                         ms_min / ms_max: the spread
  yard_ms                NOT the code under test: nq calls of the unchanged gpp_neighbourhood_quantile_fast (one scalar level each) on the same
                         cube, timed the same way and alternated with the call under test; yard_ms_min / yard_ms_max: its spread
  above_yard             ms - (yard_ms - the yardstick's spread) for nq >= 2, ms - (yard_ms + the spread) for nq == 1: the acceptance is that it
                         is not positive (many levels: below nq single calls by more than the spread; one level: no slower than the single call)
  differing_from_single  level planes that are not, bit for bit, the single-level call's (NaN with NaN): 0 or the time is worth nothing
  cdf lines              ms and its spread; gbytes_per_s: the algorithmic bytes (the cube once + Y X T floats out) over ms

  --parent-lib FILE      also times the unchanged gpp_neighbourhood_quantile_fast of another build of the library (the parent commit's) against
                         this build's, alternated in one process with the order swapped every round: lines with "variant": "single_level", parent_ms and this_ms with their spreads

Fails without a GPU.  usage: python tools/nbh_quantiles_time.py [--reps N] [--only CASE,...] [--parent-lib FILE] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--only", default="")
ap.add_argument("--parent-lib", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbh_quantiles_time.jsonl"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("nbh_quantiles_time.py: no GPU visible -- a time measured anywhere else says nothing about this path")

vp, ci = C.c_void_p, C.c_int


def load(path):
    lib = C.CDLL(path)
    lib.gpp_neighbourhood_quantile_fast.argtypes = [vp, ci, ci, ci, ci, vp, ci, ci, vp, ci, vp, ci]
    lib.gpp_last_error.restype = C.c_char_p
    return lib


L = load(os.path.join(ROOT, "gridpp_amd", "lib", "libgridpp_hip.so"))
L.gpp_neighbourhood_quantiles_fast.argtypes = [vp, ci, ci, ci, ci, vp, ci, ci, vp, ci, vp, ci]
L.gpp_neighbourhood_cdf.argtypes = [vp, ci, ci, ci, ci, ci, vp, ci, vp, ci]
PARENT = load(os.path.abspath(args.parent_lib)) if args.parent_lib else None
MEM_DEVICE, Q_HOST, WARMUP, HW, T = 1, 8, 3, 15, 11


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def ok(lib, rc):
    if rc != 0:
        sys.exit("library call failed: " + lib.gpp_last_error().decode())


def spread(t):
    return {"": round(float(np.median(t)), 4), "_min": round(min(t), 4), "_max": round(max(t), 4)}


CASES = [("config4", 4000, 4000, 100), ("tile", 530, 4000, 100)]
lines = []
for name, Y, X, E in CASES:
    if args.only and name not in args.only.split(","):
        continue
    gen = torch.Generator(device="cuda")
    gen.manual_seed(Y + X + E)
    x = torch.rand((Y, X, E), device="cuda", generator=gen) * 10
    thr = torch.linspace(0, 10, T, device="cuda")
    plane = torch.empty((Y, X), device="cuda")

    def single(lib, q):
        level = np.array([q], np.float32)
        ok(lib, lib.gpp_neighbourhood_quantile_fast(x.data_ptr(), Y, X, E, 1, level.ctypes.data, 1, HW, thr.data_ptr(), T, plane.data_ptr(), MEM_DEVICE | Q_HOST))

    for nq in (1, 3, 5, 9):
        levels = np.ascontiguousarray((np.arange(nq, dtype=np.float64) + 0.5) / nq, dtype=np.float32)
        out = torch.empty((Y, X, nq), device="cuda")

        def multi():
            ok(L, L.gpp_neighbourhood_quantiles_fast(x.data_ptr(), Y, X, E, 1, levels.ctypes.data, nq, HW, thr.data_ptr(), T, out.data_ptr(), MEM_DEVICE))

        def yard():
            for q in levels:
                single(L, float(q))

        t = {"ms": [], "yard_ms": []}
        for i in range(WARMUP + args.reps):   # alternating: the call under test and the yardstick once per round
            out.fill_(-1.0)
            for key, f in (("ms", multi), ("yard_ms", yard)):
                ms = timed(f)
                if i >= WARMUP:
                    t[key].append(ms)
        differing = 0
        for j, q in enumerate(levels):
            single(L, float(q))
            torch.cuda.synchronize()
            r = out[:, :, j]
            same = (r.contiguous().view(torch.int32) == plane.view(torch.int32)) | (torch.isnan(r) & torch.isnan(plane))
            differing += int((~same).sum())
        line = {"case": name, "Y": Y, "X": X, "E": E, "halfwidth": HW, "nt": T, "nq": nq, "variant": "levels", "reps": args.reps, "warmup": WARMUP}
        for key in t:
            line.update({key + k: v for k, v in spread(t[key]).items()})
        yard_spread = max(t["yard_ms"]) - min(t["yard_ms"])
        line["above_yard"] = round(line["ms"] - (line["yard_ms"] + yard_spread if nq == 1 else line["yard_ms"] - yard_spread), 4)
        line["differing_from_single"] = differing
        print(json.dumps(line), flush=True)
        lines.append(line)
        del out
    cdf = torch.empty((Y, X, T), device="cuda")
    t = []
    for i in range(WARMUP + args.reps):
        ms = timed(lambda: ok(L, L.gpp_neighbourhood_cdf(x.data_ptr(), Y, X, E, 1, HW, thr.data_ptr(), T, cdf.data_ptr(), MEM_DEVICE)))
        if i >= WARMUP:
            t.append(ms)
    line = {"case": name, "Y": Y, "X": X, "E": E, "halfwidth": HW, "nt": T, "variant": "cdf", "reps": args.reps, "warmup": WARMUP}
    line.update({"ms" + k: v for k, v in spread(t).items()})
    line["gbytes_per_s"] = round(4.0 * Y * X * (E + T) / (line["ms"] * 1e-3) / 1e9, 1)
    line["values_outside_0_1"] = int(((cdf < 0) | (cdf > 1)).sum())
    print(json.dumps(line), flush=True)
    lines.append(line)
    del cdf
    if PARENT is not None:   # the unchanged single-level entry point: the parent's build against this one, alternated
        t = {"parent_ms": [], "this_ms": []}
        for i in range(WARMUP + args.reps):
            for key, lib in (("parent_ms", PARENT), ("this_ms", L))[::1 if i % 2 == 0 else -1]:   # (the order swapped every round)
                ms = timed(lambda: single(lib, 0.5))
                if i >= WARMUP:
                    t[key].append(ms)
        single(PARENT, 0.5)
        torch.cuda.synchronize()
        kept = plane.clone()
        single(L, 0.5)
        torch.cuda.synchronize()
        same = (kept.view(torch.int32) == plane.view(torch.int32)) | (torch.isnan(kept) & torch.isnan(plane))
        line = {"case": name, "Y": Y, "X": X, "E": E, "halfwidth": HW, "nt": T, "nq": 1, "variant": "single_level", "reps": args.reps, "warmup": WARMUP}
        for key in t:
            line.update({key + k: v for k, v in spread(t[key]).items()})
        line["differing_from_parent"] = int((~same).sum())
        print(json.dumps(line), flush=True)
        lines.append(line)
        PARENT.gpp_release_workspaces()
    del x, plane
    torch.cuda.empty_cache()
    L.gpp_release_workspaces()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
