"""gpp_calc_ranks (ranks alone, sorted rows alone), gpp_reorder_by_ranks and gpp_calc_crps on device-resident arrays, one JSON line per
(case, function), appended to profiles/rows_rank_time.jsonl (or --out) as it is measured.  The library is called through ctypes with the
default dispatch.  Run the whole tool under one `timeout`.

  cases      4Mx50 and 1Mx160 (tile), 65536x1000 and 4096x4096 (block), 16x70001 (long: recorded, claims nothing); --only CASE,... picks some.
             Values: normal(280, 12) with 1 % NaN; the template of the reorder: another such array; ref: normal(280, 12)
  functions  calc_ranks, sort_rows, reorder_by_ranks, calc_crps

  ms           the library call, device events around a synchronised window, 3 warm-up calls, the median of 7 (--reps); ms_min / ms_max: the spread
  yard_ms      NOT the code under test: what one writes in torch today on the same tensors (NaN replaced by +inf beforehand, outside the timed
               window) -- torch.sort for sort_rows, argsort(argsort(x, stable=True)) for calc_ranks, the same plus sort and gather for
               reorder_by_ranks, sort plus the weighted sum in float64 for calc_crps -- timed the same way and alternated call by call with
               the library; yard_ms_min / yard_ms_max: its spread
  above_yard   ms - (yard_ms + the yardstick's spread yard_ms_max - yard_ms_min); the acceptance on the tile and block cases is that it is not positive
  floor_bytes  the algorithmic floor: inputs read once, outputs written once; gbytes_per_s: floor_bytes / ms
  differing    elements (rows for calc_crps: beyond 1e-5 relative) where the library and the yardstick disagree, NaN left out of the comparison

Fails without a GPU.  usage: python tools/rows_rank_time.py [--reps N] [--only CASE,...] [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_rank_time.jsonl"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("rows_rank_time.py: no GPU visible -- a time measured anywhere else says nothing about this path")

vp = C.c_void_p
L = C.CDLL(os.path.join(ROOT, "gridpp_amd", "lib", "libgridpp_hip.so"))
L.gpp_calc_ranks.argtypes = [vp, C.c_long, C.c_int, vp, vp, C.c_int]
L.gpp_reorder_by_ranks.argtypes = [vp, vp, C.c_long, C.c_int, vp, C.c_int]
L.gpp_calc_crps.argtypes = [vp, vp, C.c_long, C.c_int, vp, C.c_int]
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


def data(rows, length, gen):
    x = torch.randn((rows, length), device="cuda", generator=gen) * 12 + 280
    x[torch.rand((rows, length), device="cuda", generator=gen) < 0.01] = float("nan")
    return x


CASES = [("4Mx50", 4000000, 50, "tile"), ("1Mx160", 1000000, 160, "tile"), ("65536x1000", 65536, 1000, "block"), ("4096x4096", 4096, 4096, "block"),
         ("16x70001", 16, 70001, "long")]
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
for name, rows, length, path in CASES:
    if args.only and name not in args.only.split(","):
        continue
    gen = torch.Generator(device="cuda")
    gen.manual_seed(rows + length)
    x, tm = data(rows, length, gen), data(rows, length, gen)
    y = torch.randn(rows, device="cuda", generator=gen) * 12 + 280
    xi, ti = torch.nan_to_num(x, nan=float("inf")), torch.nan_to_num(tm, nan=float("inf"))   # the torch side: NaN -> +inf, sorted last
    n = rows * length
    ranks, fout, rout = torch.empty((rows, length), dtype=torch.int32, device="cuda"), torch.empty((rows, length), device="cuda"), torch.empty(rows, device="cuda")
    keep = {}

    def torch_ranks(a):
        return torch.argsort(torch.argsort(a, dim=-1, stable=True), dim=-1)

    def yard_crps():
        s = torch.sort(xi, dim=-1).values.to(torch.float64)
        w = 2 * torch.arange(length, device="cuda", dtype=torch.float64) - length + 1
        return (s - y.to(torch.float64)[:, None]).abs().mean(-1) - (s * w).sum(-1) / (float(length) * length)

    FUNCS = {
        "calc_ranks": (lambda: ok(L.gpp_calc_ranks(x.data_ptr(), rows, length, ranks.data_ptr(), None, MEM_DEVICE)), lambda: torch_ranks(xi), 8 * n),
        "sort_rows": (lambda: ok(L.gpp_calc_ranks(x.data_ptr(), rows, length, None, fout.data_ptr(), MEM_DEVICE)), lambda: torch.sort(xi, dim=-1).values, 8 * n),
        "reorder_by_ranks": (lambda: ok(L.gpp_reorder_by_ranks(x.data_ptr(), tm.data_ptr(), rows, length, fout.data_ptr(), MEM_DEVICE)),
                             lambda: torch.gather(torch.sort(xi, dim=-1).values, -1, torch_ranks(ti)), 12 * n),
        "calc_crps": (lambda: ok(L.gpp_calc_crps(x.data_ptr(), y.data_ptr(), rows, length, rout.data_ptr(), MEM_DEVICE)), yard_crps, 4 * n + 8 * rows),
    }
    for fn, (ours, yard, floor) in FUNCS.items():
        t = {"ours": [], "yard": []}

        def run_yard():
            keep["yard"] = yard()

        for i in range(WARMUP + args.reps):   # alternating call by call
            a, b = timed(ours), timed(run_yard)
            if i >= WARMUP:
                t["ours"].append(a)
                t["yard"].append(b)
        want = keep.pop("yard")
        if fn == "calc_ranks":
            differing = int(((ranks.long() != want) & ~torch.isnan(x)).sum())
        elif fn == "calc_crps":
            full = ~torch.isnan(x).any(-1)
            differing = int((((rout.double() - want).abs() > 1e-5 * want.abs()) & full).sum())
        else:
            differing = int(((fout != want) & ~torch.isnan(fout)).sum())
        del want
        ms, ym = float(np.median(t["ours"])), float(np.median(t["yard"]))
        line = {"case": name, "rows": rows, "len": length, "path": path, "function": fn, "ms": round(ms, 4), "ms_min": round(min(t["ours"]), 4),
                "ms_max": round(max(t["ours"]), 4), "reps": len(t["ours"]), "warmup": WARMUP, "yard_ms": round(ym, 4), "yard_ms_min": round(min(t["yard"]), 4),
                "yard_ms_max": round(max(t["yard"]), 4), "above_yard": round(ms - (ym + max(t["yard"]) - min(t["yard"])), 4), "floor_bytes": floor,
                "gbytes_per_s": round(floor / ms / 1e6, 1), "differing": differing}
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    del x, tm, xi, ti, ranks, fout, rout, y
    torch.cuda.empty_cache()
    L.gpp_release_workspaces()
