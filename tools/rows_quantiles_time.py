"""gpp_calc_quantiles on device-resident arrays, one JSON line per (case, number of levels, variant), appended to
profiles/rows_quantiles_time.jsonl (or --out).  The library is called through ctypes.

  cases      4Mx50 and 1Mx160 with 1, 2, 3, 5, 11 and 101 levels; 65536x1000, 4096x4096 and 16x70001 (the loop path) with 5 and 101;
             --extra ROWSxLENxNQ,... adds cases (the sweeps that set the gates).  Values: normal(280, 12) with 1 % NaN; levels: evenly
             spaced inside (0, 1), so that no call pays the walk for the positional Min / Max
  variants   default (the dispatch) and tile / block / loop forced with GPP_ROWS_QUANTILES where the path applies

  ms                  the library call, device events around a synchronised window, 3 warm-up calls, the median of 7 (--reps); ms_min / ms_max: the spread
  yard_ms             NOT the code under test: nq calls of gpp_calc_quantile (one scalar level each, its own dispatch) and a device-to-device copy of
                      the input's + the output's bytes, timed the same way and alternated with the variants; yard_ms_min / yard_ms_max: its spread
  above_yard          default only: ms - (yard_ms + the yardstick's spread yard_ms_max - yard_ms_min); the acceptance is that it is not positive
  differing_from_loop results that are not, bit for bit, the loop path's (NaN with NaN): 0 or the time is worth nothing

Fails without a GPU.  usage: python tools/rows_quantiles_time.py [--reps N] [--only CASE,...] [--extra ROWSxLENxNQ,...] [--out FILE]"""
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
ap.add_argument("--extra", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_quantiles_time.jsonl"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("rows_quantiles_time.py: no GPU visible -- a time measured anywhere else says nothing about this path")

vp = C.c_void_p
L = C.CDLL(os.path.join(ROOT, "gridpp_amd", "lib", "libgridpp_hip.so"))
L.gpp_calc_quantiles.argtypes = [vp, C.c_long, C.c_int, vp, C.c_int, vp, C.c_int]
L.gpp_calc_quantile.argtypes = [vp, C.c_long, C.c_int, vp, C.c_long, vp, C.c_int]
L.gpp_set_path_override.argtypes = [C.c_char_p, C.c_char_p]
L.gpp_last_error.restype = C.c_char_p
MEM_DEVICE, WARMUP = 1, 3


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def ok(rc):
    if rc != 0:
        sys.exit("library call failed: " + L.gpp_last_error().decode())


FEW, TWO = (1, 2, 3, 5, 11, 101), (5, 101)
CASES = [("4Mx50", 4000000, 50, FEW), ("1Mx160", 1000000, 160, FEW), ("65536x1000", 65536, 1000, TWO), ("4096x4096", 4096, 4096, TWO),
         ("16x70001", 16, 70001, TWO)]
for e in [e for e in args.extra.split(",") if e]:
    r, n, k = (int(x) for x in e.split("x"))
    CASES.append(("%dx%d" % (r, n), r, n, (k,)))
EXTRA = len([e for e in args.extra.split(",") if e])

lines = []
for ci, (name, rows, length, counts) in enumerate(CASES):
    if args.only and ci < len(CASES) - EXTRA and name not in args.only.split(","):   # (--only none: the extra cases alone)
        continue
    gen = torch.Generator(device="cuda")
    gen.manual_seed(rows + length)
    x = torch.randn((rows, length), device="cuda", generator=gen) * 12 + 280
    x[torch.rand((rows, length), device="cuda", generator=gen) < 0.01] = float("nan")
    for nq in counts:
        levels = np.ascontiguousarray((np.arange(nq, dtype=np.float64) + 0.5) / nq, dtype=np.float32)
        dlevels = torch.from_numpy(levels).cuda()
        out, column = torch.empty((rows, nq), device="cuda"), torch.empty(rows, device="cuda")
        src, dst = torch.empty(rows * (length + nq), device="cuda"), torch.empty(rows * (length + nq), device="cuda")
        applies = {"default": True, "tile": nq > 1 and length <= 160, "block": nq > 1 and 160 < length <= 8192, "loop": True}
        variants = [v for v in ("default", "tile", "block", "loop") if applies[v]]
        results, t = {}, {v: [] for v in variants + ["yard"]}

        def run(v):
            if v != "default":
                L.gpp_set_path_override(b"GPP_ROWS_QUANTILES", v.encode())
            try:
                out.fill_(-1.0)
                ms = timed(lambda: ok(L.gpp_calc_quantiles(x.data_ptr(), rows, length, levels.ctypes.data, nq, out.data_ptr(), MEM_DEVICE)))
                results[v] = out.clone()
            finally:
                L.gpp_set_path_override(b"GPP_ROWS_QUANTILES", None)
            return ms

        def yard():
            for j in range(nq):
                ok(L.gpp_calc_quantile(x.data_ptr(), rows, length, dlevels[j:].data_ptr(), 1, column.data_ptr(), MEM_DEVICE))
            dst.copy_(src)

        for i in range(WARMUP + args.reps):   # alternating: every variant and the yardstick once per round
            for v in variants:
                ms = run(v)
                if i >= WARMUP:
                    t[v].append(ms)
            ms = timed(yard)
            if i >= WARMUP:
                t["yard"].append(ms)
        ref = results["loop"]
        for v in variants:
            r = results[v]
            same = (r.view(torch.int32) == ref.view(torch.int32)) | (torch.isnan(r) & torch.isnan(ref))
            ms = float(np.median(t[v]))
            line = {"case": name, "rows": rows, "len": length, "nq": nq, "variant": v, "ms": round(ms, 4), "ms_min": round(min(t[v]), 4),
                    "ms_max": round(max(t[v]), 4), "reps": len(t[v]), "warmup": WARMUP, "yard_ms": round(float(np.median(t["yard"])), 4),
                    "yard_ms_min": round(min(t["yard"]), 4), "yard_ms_max": round(max(t["yard"]), 4), "differing_from_loop": int((~same).sum())}
            if v == "default":
                line["above_yard"] = round(ms - (float(np.median(t["yard"])) + max(t["yard"]) - min(t["yard"])), 4)
            print(json.dumps(line), flush=True)
            lines.append(line)
        del out, column, src, dst
    del x
    torch.cuda.empty_cache()
    L.gpp_release_workspaces()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
