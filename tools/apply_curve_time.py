"""apply_curve on device-resident tensors, one JSON line per case (appended to profiles/apply_curve_time.jsonl, or --out):

  shared_2000x2000_nc2000    one curve of 2000 entries for a 2000 x 2000 field (the reference's tests/benchmark.py row)
  shared_4000x4000_nc100     one curve of 100 entries for a 4000 x 4000 field
  field_2000x2000_nc10       one curve per cell, 2000 x 2000 x 10 (the reference's "gridded" row)
  field_4000x4000_nc50       one curve per cell, 4000 x 4000 x 50: 6.4 GB of curves, far beyond the 256 MiB cache

  fused_ms       the library call (gridpp.apply_curve on torch CUDA tensors), device events around a synchronised window, warmed up;
                 median, minimum and maximum of the repetitions
  yardstick_ms   NOT the code under test: the composed device path a user has without these entry points -- torch.searchsorted on
                 curve_fcst, four gathers and the lerp in torch.  It is valid for sorted, duplicate-free, NaN-free curves and
                 in-range inputs, which is what the cases use; allclose against the fused result is checked on exactly those inputs.
                 Measured in the same process, alternated with the fused call.
  bytes          what the algorithm needs, from the shapes: 8 n (shared curve), (2 nc + 2) * 4 * ny * nx (curve per cell)
  share_of_8.0TBps / share_of_6.29TBps   bytes / fused time over the HBM3E figure DESIGN.md uses and over the float4-copy rate
                 measured on this chip (the practical ceiling)
  not_slower     fused median <= yardstick median + the spread (max - min) of the alternated repetitions of both

Fails without a GPU.  usage: python tools/apply_curve_time.py [--reps N] [--only NAME,...] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import gridpp_amd as gridpp

PEAK, COPY_RATE = 8.0e12, 6.29e12

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--only", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "apply_curve_time.jsonl"))
args = ap.parse_args()

if not torch.cuda.is_available() or gridpp.device_count() == 0:
    sys.exit("apply_curve_time.py: no GPU visible -- a time measured anywhere else says nothing about this path")


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def increasing(shape, gen):
    """strictly increasing along the last axis: no duplicates, no NaN"""
    return torch.rand(shape, device="cuda", generator=gen).add_(0.01).cumsum_(-1)


def inputs_between(cf, shape, gen):
    u = torch.rand(shape, device="cuda", generator=gen) * 0.98 + 0.01
    return cf[..., 0] + u * (cf[..., -1] - cf[..., 0])


def composed_shared(x, cr, cf):
    nc = cf.shape[0]
    i1 = torch.searchsorted(cf, x).clamp_(1, nc - 1)
    i0 = i1 - 1
    x0, x1, y0, y1 = cf[i0], cf[i1], cr[i0], cr[i1]
    return y0 + (y1 - y0) * (x - x0) / (x1 - x0)


def composed_field(x, cr, cf):
    nc = cf.shape[-1]
    i1 = torch.searchsorted(cf, x.unsqueeze(-1)).clamp_(1, nc - 1)
    i0 = i1 - 1
    x0, x1, y0, y1 = (torch.gather(c, -1, i).squeeze(-1) for c, i in ((cf, i0), (cf, i1), (cr, i0), (cr, i1)))
    return y0 + (y1 - y0) * (x - x0) / (x1 - x0)


CASES = (("shared_2000x2000_nc2000", False, 2000, 2000, 2000), ("shared_4000x4000_nc100", False, 4000, 4000, 100),
         ("field_2000x2000_nc10", True, 2000, 2000, 10), ("field_4000x4000_nc50", True, 4000, 4000, 50))

lines = []
for case, per_cell, ny, nx, nc in CASES:
    if args.only and case not in args.only.split(","):
        continue
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234 + nc)
    cshape = (ny, nx, nc) if per_cell else (nc,)
    cf, cr = increasing(cshape, gen), increasing(cshape, gen)
    x = inputs_between(cf, (ny, nx), gen)
    if per_cell:
        def fused():
            return gridpp.apply_curve(x, cr, cf, gridpp.OneToOne, gridpp.OneToOne)

        def yardstick():
            return composed_field(x, cr, cf)
        nbytes = (2 * nc + 2) * 4 * ny * nx
    else:
        cr_h, cf_h = cr.cpu().numpy(), cf.cpu().numpy()   # the shared curve is a host array of the call

        def fused():
            return gridpp.apply_curve(x, cr_h, cf_h, gridpp.OneToOne, gridpp.OneToOne)

        def yardstick():
            return composed_shared(x, cr, cf)
        nbytes = 8 * ny * nx
    a, b = fused(), yardstick()   # (warm-up of both, and the proof that the two do the same job on these inputs)
    same = bool(torch.allclose(a, b, rtol=1e-4, atol=1e-5))
    worst = float((a - b).abs().max())
    del a, b
    for _ in range(2):
        fused()
        yardstick()
    tf, ty = [], []
    for _ in range(args.reps):
        tf.append(timed(fused))
        ty.append(timed(yardstick))
    f_ms, y_ms = float(np.median(tf)), float(np.median(ty))
    spread = (max(tf) - min(tf)) + (max(ty) - min(ty))
    line = {"case": case, "shape": [ny, nx], "nc": nc, "curve_per_cell": per_cell, "fused_ms": round(f_ms, 3), "fused_ms_min": round(min(tf), 3),
            "fused_ms_max": round(max(tf), 3), "yardstick_ms": round(y_ms, 3), "yardstick_ms_min": round(min(ty), 3), "yardstick_ms_max": round(max(ty), 3),
            "yardstick": "torch.searchsorted + gathers + lerp", "speedup": round(y_ms / f_ms, 2), "bytes": nbytes,
            "share_of_8.0TBps": round(nbytes / PEAK / (f_ms / 1e3), 4), "share_of_6.29TBps": round(nbytes / COPY_RATE / (f_ms / 1e3), 4),
            "allclose_to_yardstick": same, "max_abs_difference": worst, "not_slower": bool(f_ms <= y_ms + spread), "spread_ms": round(spread, 3),
            "reps": args.reps}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del cf, cr, x
    torch.cuda.empty_cache()

with open(args.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
