"""gpp_calc_quantile on device-resident arrays, one JSON line per (case, level form, library / forced path), appended to
profiles/rows_quantile_time.jsonl (or --out).  The library is called through ctypes, so the same script times another build of it
(--parent FILE: the library of the parent commit) in the same process, alternated call by call with the one of this tree.

  cases      4Mx50 (a 2000 x 2000 cube of 50 members), 1Mx160, 65536x1000, 4096x4096, 8x2^21, 1x2^20, and 1x2^24 (this tree only: the
             parent runs it on one lane with up to 64 walks of the row); --extra adds shapes (this tree only), for the sweeps that set the gates
  levels     scalar: q = 0.5 for every row; field: one level per row (uniform in [0, 1])
  variants   new (the default dispatch), parent, and new:<path> with GPP_ROWS_SELECT forced (--paths lane,tile,block,split: only where
             the path applies and, for lane, where one call stays short)

  ms            the library call, device events around a synchronised window, warmed up; median, minimum and maximum of the repetitions
  copy_ms       NOT the code under test: a device-to-device copy of the array's bytes, alternated with the calls
  mean_ms       NOT the code under test (rows of up to 160 values): gpp_calc_statistic(Mean) on the same array, the LDS-staged member pass
  sort_ms       NOT the code under test (one-row cases): gpp_calc_even_quantiles on the same values -- the rocPRIM radix sort (+ unique) a
                sort-based split path would have to run
  GBps          4 bytes per value over ms (what one read of the array needs)
  rows_differing_from_new   rows whose result is not, bit for bit, the default dispatch's (NaN with NaN): 0 or the time is worth nothing

Fails without a GPU.  usage: python tools/rows_quantile_time.py [--parent FILE] [--paths P,...] [--reps N] [--only CASE,...] [--extra ROWSxLEN,...] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--only", default="")
ap.add_argument("--parent", default="")
ap.add_argument("--paths", default="")
ap.add_argument("--extra", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_quantile_time.jsonl"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("rows_quantile_time.py: no GPU visible -- a time measured anywhere else says nothing about this path")

vp = C.c_void_p


def load(path):
    L = C.CDLL(path)
    L.gpp_calc_quantile.argtypes = [vp, C.c_long, C.c_int, vp, C.c_long, vp, C.c_int]
    L.gpp_calc_statistic.argtypes = [vp, C.c_long, C.c_int, C.c_int, vp, C.c_int]
    L.gpp_calc_even_quantiles.argtypes = [vp, C.c_long, C.c_int, C.c_int, vp, C.POINTER(C.c_int), C.c_int]
    L.gpp_set_path_override.argtypes = [C.c_char_p, C.c_char_p]
    L.gpp_last_error.restype = C.c_char_p
    return L


NEW = load(os.path.join(ROOT, "gridpp_amd", "lib", "libgridpp_hip.so"))
PARENT = load(os.path.abspath(args.parent)) if args.parent else None
MEM_DEVICE, MEAN = 1, 0


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def ok(L, rc):
    if rc != 0:
        sys.exit("library call failed: " + L.gpp_last_error().decode())


CASES = (("4Mx50", 4000000, 50, True), ("1Mx160", 1000000, 160, True), ("65536x1000", 65536, 1000, True), ("4096x4096", 4096, 4096, True),
         ("8x2^21", 8, 1 << 21, True), ("1x2^20", 1, 1 << 20, True), ("1x2^24", 1, 1 << 24, False))   # name, rows, len, parent runs it
CASES += tuple((e, int(e.split("x")[0]), int(e.split("x")[1]), False) for e in args.extra.split(",") if e)   # --extra ROWSxLEN,...: the gate sweeps
LANE_MAX_LEN = 4096   # forced lane path: only where a call stays short

lines = []
for name, rows, length, with_parent in CASES:
    if args.only and name not in args.only.split(","):
        continue
    gen = torch.Generator(device="cuda")
    gen.manual_seed(rows + length)
    x = torch.randn((rows, length), device="cuda", generator=gen) * 12 + 280   # temperature-like values
    x[torch.rand((rows, length), device="cuda", generator=gen) < 0.01] = float("nan")
    spare = torch.empty_like(x)
    out = torch.empty(rows, device="cuda")
    levels = {"scalar": torch.full((1,), 0.5, device="cuda"), "field": torch.rand(rows, device="cuda", generator=gen)}

    def copy():
        spare.copy_(x)

    def quantile(L, q):
        ok(L, L.gpp_calc_quantile(x.data_ptr(), rows, length, q.data_ptr(), q.numel(), out.data_ptr(), MEM_DEVICE))

    for form, q in levels.items():
        variants = [("new", NEW, None)]
        if PARENT is not None and with_parent:
            variants.append(("parent", PARENT, None))
        for p in [p for p in args.paths.split(",") if p]:
            applies = {"lane": length <= LANE_MAX_LEN, "tile": length <= 160, "block": True, "split": rows <= 65535}[p]
            if applies:
                variants.append(("new:" + p, NEW, p))
        yard = {"copy": copy}
        if length <= 160:
            yard["mean"] = lambda: ok(NEW, NEW.gpp_calc_statistic(x.data_ptr(), rows, length, MEAN, out.data_ptr(), MEM_DEVICE))
        if rows == 1:
            eq_out, eq_n = torch.empty(16, device="cuda"), C.c_int(0)
            yard["sort"] = lambda: ok(NEW, NEW.gpp_calc_even_quantiles(x.data_ptr(), rows * length, 16, 1, eq_out.data_ptr(), C.byref(eq_n), MEM_DEVICE))
        results, t = {}, {}

        def run(v):
            vname, L, path = v
            if path:
                L.gpp_set_path_override(b"GPP_ROWS_SELECT", path.encode())
            try:
                ms = timed(lambda: quantile(L, q))
                results[vname] = out.clone()
            finally:
                if path:
                    L.gpp_set_path_override(b"GPP_ROWS_SELECT", None)
            return ms

        first = {v[0]: run(v) for v in variants}   # (loads the code objects; says which variants are slow)
        # a variant whose call takes seconds (one lane walking a long row) is not repeated: its first call is its time
        nrep = {k: 0 if ms > 2000 else 3 if ms > 200 else args.reps for k, ms in first.items()}
        nwarm = {k: 2 if n == args.reps else 0 for k, n in nrep.items()}
        for i in range(2):
            for v in variants:
                if i < nwarm[v[0]]:
                    run(v)
            for f in yard.values():
                f()
        for i in range(args.reps):   # alternating: every variant and yardstick once per round
            for v in variants:
                if i < nrep[v[0]]:
                    t.setdefault(v[0], []).append(run(v))
            for k, f in yard.items():
                t.setdefault(k, []).append(timed(f))
        for k, ms in first.items():
            t.setdefault(k, [ms])
        # the variants must agree bit for bit (NaN with NaN) before a time is worth anything
        ref = results["new"].view(torch.int32)
        differ = {}
        for vname, r in results.items():
            same = (r.view(torch.int32) == ref) | (torch.isnan(r) & torch.isnan(results["new"]))
            differ[vname] = int((~same).sum())
        for vname, _, path in variants:
            ms = float(np.median(t[vname]))
            line = {"case": name, "rows": rows, "len": length, "levels": form, "variant": vname, "ms": round(ms, 4), "ms_min": round(min(t[vname]), 4),
                    "ms_max": round(max(t[vname]), 4), "reps": len(t[vname]), "warmup": (1 + nwarm[vname]) if nrep[vname] else 0, "bytes": 4 * rows * length,
                    "GBps": round(4 * rows * length / (ms / 1e3) / 1e9, 1), "rows_differing_from_new": differ[vname]}
            for k in yard:
                line[k + "_ms"] = round(float(np.median(t[k])), 4)
                line[k + "_ms_min"], line[k + "_ms_max"] = round(min(t[k]), 4), round(max(t[k]), 4)
            print(json.dumps(line), flush=True)
            lines.append(line)
    del x, spare, out, levels
    torch.cuda.empty_cache()
    NEW.gpp_release_workspaces()
    if PARENT is not None:
        PARENT.gpp_release_workspaces()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
