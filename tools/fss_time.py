"""gridpp_amd.fractions_skill_score on device-resident fields against the composition users write today, one JSON line per (case, set
of half widths), appended to profiles/fss_time.jsonl (or --out).

  cases      field (4000 x 4000 against 4000 x 4000) and cube (4000 x 4000 x 50 against 4000 x 4000): a smooth pattern plus noise, every value
             valid, five thresholds (-1, -0.5, 0, 0.5, 1), operator Gt; one line per half width 1, 2, 4, 8, 16, 32 (all five thresholds in one
             call) and one line for the whole 5 x 6 table in one call

  ms         one fractions_skill_score call on torch device tensors, device events around a synchronised window, 3 warm-up rounds, the
             median of 7 (--reps); ms_min / ms_max: the spread
  comp_ms    NOT the code under test, and unchanged by it: the same numbers composed from calls that exist without it -- per threshold the
             0/1 plane of ref and the 0/1 plane of fcst (cube: the member fraction (cube > t).sum(2) / E) in torch, per half width two
             gridpp_amd.neighbourhood(plane, h, Mean) calls and the two sums in torch float64 -- timed the same way and alternated with the
             call under test round by round; comp_ms_min / comp_ms_max: its spread
  ratio      comp_ms / ms
  win        whether comp_ms - ms exceeds the sum of the two spreads (max - min each): only then does a line count as faster
  max_abs_fss_diff   the largest |fss - composed fss| of the line: the composition rounds its fractions to float32, so up to about 2^-22

  --no-comp  times the call under test alone (for a kernel trace of it)

Fails without a GPU.  usage: python tools/fss_time.py [--reps N] [--only CASE,...] [--no-comp] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--only", default="")
ap.add_argument("--no-comp", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fss_time.jsonl"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("fss_time.py: no GPU visible -- a time measured anywhere else says nothing about this path")

import gridpp_amd as gridpp

WARMUP = 3
THR = [-1.0, -0.5, 0.0, 0.5, 1.0]
HWS = [1, 2, 4, 8, 16, 32]


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def spread(t):
    return {"": round(float(np.median(t)), 4), "_min": round(min(t), 4), "_max": round(max(t), 4)}


def composed(fcst, ref, hws):
    """the (T, H) table of fss from existing calls; every value of the timing cases is valid, so no cell is masked out"""
    sums = torch.zeros((len(THR), len(hws), 2), dtype=torch.float64, device="cuda")
    for t, th in enumerate(THR):
        pf = (fcst > th).float() if fcst.dim() == 2 else (fcst > th).sum(2, dtype=torch.float32) / fcst.shape[2]
        po = (ref > th).float()
        for j, h in enumerate(hws):
            mf, mo = gridpp.neighbourhood(pf, h, gridpp.Mean).double(), gridpp.neighbourhood(po, h, gridpp.Mean).double()
            sums[t, j, 0] = ((mf - mo) ** 2).sum()
            sums[t, j, 1] = (mf ** 2 + mo ** 2).sum()
    s = sums.cpu().numpy()
    return 1.0 - s[:, :, 0] / s[:, :, 1]


lines = []
for name, Y, X, E in (("field", 4000, 4000, 1), ("cube", 4000, 4000, 50)):
    if args.only and name not in args.only.split(","):
        continue
    gen = torch.Generator(device="cuda")
    gen.manual_seed(Y + X + E)
    yy, xx = torch.meshgrid(torch.arange(Y, device="cuda") / 90.0, torch.arange(X, device="cuda") / 130.0, indexing="ij")
    smooth = torch.sin(yy) + torch.cos(xx)
    ref = smooth + 0.5 * torch.randn((Y, X), device="cuda", generator=gen)
    if E == 1:
        fcst = smooth + 0.5 * torch.randn((Y, X), device="cuda", generator=gen)
    else:
        fcst = torch.randn((Y, X, E), device="cuda", generator=gen)
        fcst.mul_(0.5).add_(smooth[:, :, None])
    del yy, xx, smooth
    for hws in [[h] for h in HWS] + [HWS]:
        t = {"ms": [], "comp_ms": []}
        got = comp = None
        for i in range(WARMUP + args.reps):   # alternating: the call under test and the composition once per round
            ms, got = timed(lambda: gridpp.fractions_skill_score(fcst, ref, THR, hws))
            if i >= WARMUP:
                t["ms"].append(ms)
            if not args.no_comp:
                ms, comp = timed(lambda: composed(fcst, ref, hws))
                if i >= WARMUP:
                    t["comp_ms"].append(ms)
        line = {"case": name, "Y": Y, "X": X, "E": E, "nt": len(THR), "halfwidths": hws, "reps": args.reps, "warmup": WARMUP}
        line.update({"ms" + k: v for k, v in spread(t["ms"]).items()})
        if not args.no_comp:
            line.update({"comp_ms" + k: v for k, v in spread(t["comp_ms"]).items()})
            line["ratio"] = round(line["comp_ms"] / line["ms"], 2)
            line["win"] = bool(line["comp_ms"] - line["ms"] > (max(t["ms"]) - min(t["ms"])) + (max(t["comp_ms"]) - min(t["comp_ms"])))
            line["max_abs_fss_diff"] = float(np.max(np.abs(got.fss - comp)))
        line["fss_first_threshold"] = [round(float(v), 6) for v in got.fss[0]]
        print(json.dumps(line), flush=True)
        lines.append(line)
    del fcst, ref
    torch.cuda.empty_cache()
    gridpp.release_workspaces() if hasattr(gridpp, "release_workspaces") else None

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
