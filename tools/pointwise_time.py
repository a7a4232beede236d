"""The weather diagnostics and the value transforms on device-resident tensors of 4000 x 4000 values, one JSON line per function
(appended to profiles/pointwise_time.jsonl, or --out):

  fused_ms       the library call (gridpp.<function> on torch CUDA tensors), device events around a synchronised window, warmed up;
                 median, minimum and maximum of the repetitions
  yardstick_ms   NOT the code under test: the composed device path a user had before these entry points -- the same formula in torch,
                 float64 math, cast to float32 at the end.  It writes and re-reads every intermediate through HBM.  It is valid for the
                 clean physical inputs the cases use (no missing values, none of the reference's special cases); allclose against the
                 fused result is checked on exactly those inputs.  Measured in the same process, alternated with the fused call.
  bytes          what the algorithm needs, from the shapes: 4 (NIN + 1) bytes per value
  gbps           bytes / fused median
  share_of_copy  gbps over the copy rate measured in this run the way tools/bw_probe.py measures it (torch's clone of a tensor far
                 beyond the cache, read + write bytes over the best of five): the practical ceiling of a streaming kernel
  not_slower     fused median <= yardstick median + the spread (max - min) of the alternated repetitions of both

Fails without a GPU.  usage: python tools/pointwise_time.py [--reps N] [--only NAME,...] [--out FILE]"""
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
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--only", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointwise_time.jsonl"))
ap.add_argument("--side", type=int, default=4000)
args = ap.parse_args()

if not torch.cuda.is_available() or gridpp.device_count() == 0:
    sys.exit("pointwise_time.py: no GPU visible -- a time measured anywhere else says nothing about this path")

N = args.side * args.side
gen = torch.Generator(device="cuda")
gen.manual_seed(4242)


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def uniform(lo, hi):
    return torch.rand(N, device="cuda", generator=gen) * (hi - lo) + lo


def copy_rate():
    """bytes per second of torch's clone (read + write), as tools/bw_probe.py takes it"""
    big = torch.rand((args.side, args.side, 25), device="cuda", generator=gen)
    big.clone()
    best = min(timed(big.clone) for _ in range(5))
    return 2 * big.numel() * 4 / (best / 1e3)


EWT = torch.tensor([.000034, .000089, .000220, .000517, .001155, .002472, .005080, .01005, .01921, .03553, .06356, .1111, .1891, .3139, .5088, .8070, 1.2540,
                    1.9118, 2.8627, 4.2148, 6.1078, 8.7192, 12.272, 17.044, 23.373, 31.671, 42.430, 56.236, 73.777, 95.855, 123.40, 157.46, 199.26, 250.16,
                    311.69, 385.56, 473.67, 578.09, 701.13, 845.28, 1013.25], dtype=torch.float64, device="cuda")


def t_dewpoint(t, rh):
    t, rh = t.double(), rh.double()
    tc = t - 273.15
    le = torch.log(rh * 0.611 * torch.exp(17.63 * tc / (tc + 243.04)))
    return torch.minimum((116.9 + 243.04 * le) / (16.78 - le) + 273.15, t).float()


def t_ewt(k):
    x = ((k.double() - 173.16) * 0.2).clamp_(0, 39)
    i = x.floor().long()
    return EWT[i] + (EWT[i + 1] - EWT[i]) * (x - i)


def t_relative_humidity(t, td):
    return torch.where(t <= td, 1.0, (t_ewt(td) / t_ewt(t)).clamp_(0, 1)).float()


def t_wetbulb(t, p, rh):
    tc = t.double() - 273.15
    e = rh.double() * 0.611 * torch.exp(17.63 * tc / (tc + 243.04))
    le = torch.log(e)
    td = (116.9 + 243.04 * le) / (16.78 - le)
    gamma = 0.00066 * p.double() / 1000
    delta = 4098 * e / (td + 243.04) ** 2
    return ((gamma * tc + delta * td) / (gamma + delta) + 273.15).float()


def t_pressure(ie, oe, ip, it):
    return (ip.double() * torch.exp(-9.80665 * 0.0289644 * (oe.double() - ie.double()) / (8.3144598 * it.double()))).float()


def t_sea_level_pressure(ps, alt, t, rh, dew):   # the relative humidity branch (every rh of the case is valid)
    T, ps, alt = t.double() - 273.15, ps.double() * 0.01, alt.double()
    e = rh.double() * 6.11 * torch.pow(10., 7.5 * T / (237.3 + T))
    le = torch.log(e / 6.1094)
    d = 243.04 * le / (17.625 - le)
    high = ps * torch.exp((9.80665 * alt / 287.05) / (273.15 + T + 0.5 * 0.0065 * alt + e * 0.12))
    tv = (273.15 + T) / (1 - 0.379 * (6.11 * torch.pow(10., 7.5 * d / (237.7 + d)) / ps))
    return (torch.where(alt >= 50, high, ps + ps * alt / (29.27 * tv)) * 100).float()


def t_qnh(p, alt):
    g, T0, L, CR, p0 = 9.80665, 288.15, 0.0065, 287.053, 101325.0
    return (p0 * torch.pow(torch.pow(p.double() / p0, CR * L / g) + alt.double() * L / T0, g / (CR * L))).float()


def t_wind_speed(x, y):
    return torch.sqrt(x.double() ** 2 + y.double() ** 2).float()


def t_wind_direction(x, y):
    d = torch.atan2(-x.double(), -y.double()) * 180 / np.pi
    return torch.where(d < 0, d + 360, d).float()


def t_boxcox_forward(v, thr=0.1):
    return ((torch.pow(v.double().clamp_(min=0), thr) - 1) / thr).float()


def t_boxcox_backward(v, thr=0.1):
    return torch.pow(1 + thr * v.double().clamp_(min=-1 / thr), 1 / thr).clamp_(min=0).float()


def t_started_forward(v, thr=0.3, s=2.5):
    v = v.double().clamp_(min=0)
    return torch.where(v <= s, v, s * (1 + (torch.pow(v / s, thr) - 1) / thr)).float()


def t_started_backward(v, thr=0.3, s=2.5):
    v = v.double()
    return torch.where(v <= s, v, s * torch.pow(1 + thr / s * (v - s).clamp_(min=0), 1 / thr)).clamp_(min=0).float()


def cases():
    t = lambda: uniform(230, 320)
    precip = lambda: uniform(0, 40)
    yield "dewpoint", gridpp.dewpoint, t_dewpoint, lambda: (t(), uniform(0.05, 1))
    yield "relative_humidity", gridpp.relative_humidity, t_relative_humidity, lambda: (lambda a: (a, a - uniform(0, 30)))(t())
    yield "wetbulb", gridpp.wetbulb, t_wetbulb, lambda: (t(), uniform(50000, 105000), uniform(0.05, 1))
    yield "pressure", gridpp.pressure, t_pressure, lambda: (uniform(0, 3000), uniform(0, 3000), uniform(60000, 105000), t())
    yield ("sea_level_pressure", gridpp.sea_level_pressure, t_sea_level_pressure,
           lambda: (uniform(60000, 105000), uniform(-100, 3000), t(), uniform(0.05, 1), torch.full((N,), float("nan"), device="cuda")))
    yield "qnh", gridpp.qnh, t_qnh, lambda: (uniform(60000, 105000), uniform(0, 3000))
    yield "wind_speed", gridpp.wind_speed, t_wind_speed, lambda: (uniform(-30, 30), uniform(-30, 30))
    yield "wind_direction", gridpp.wind_direction, t_wind_direction, lambda: (uniform(-30, 30), uniform(-30, 30))
    yield "Identity.forward", gridpp.Identity().forward, torch.clone, lambda: (precip(),)
    yield "Log.forward", gridpp.Log().forward, lambda v: torch.log(v.double()).float(), lambda: (uniform(0.01, 40),)
    yield "Log.backward", gridpp.Log().backward, lambda v: torch.exp(v.double()).float(), lambda: (uniform(-5, 5),)
    yield "BoxCox(0.1).forward", gridpp.BoxCox(0.1).forward, t_boxcox_forward, lambda: (precip(),)
    yield "BoxCox(0.1).backward", gridpp.BoxCox(0.1).backward, t_boxcox_backward, lambda: (uniform(-10, 5),)
    yield "StartedBoxCox(0.3, 2.5).forward", gridpp.StartedBoxCox(0.3, 2.5).forward, t_started_forward, lambda: (precip(),)
    yield "StartedBoxCox(0.3, 2.5).backward", gridpp.StartedBoxCox(0.3, 2.5).backward, t_started_backward, lambda: (uniform(0, 12),)


rate = copy_rate()
print(json.dumps({"copy_rate_gbps": round(rate / 1e9, 1), "how": "torch clone of %d x %d x 25 float32, read + write, best of 5" % (args.side, args.side)}), flush=True)
lines = []
for name, fused_fn, yard_fn, make in cases():
    if args.only and name not in args.only.split(","):
        continue
    inputs = make()

    def fused():
        return fused_fn(*inputs)

    def yardstick():
        return yard_fn(*inputs)
    a, b = fused(), yardstick()   # (warm-up of both, and the proof that the two do the same job on these inputs)
    same = bool(torch.allclose(a, b, rtol=1e-4, atol=1e-5, equal_nan=True))
    worst = float(((a - b).abs() / b.abs().clamp_(min=1e-3)).max())
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
    nbytes = 4 * (len(inputs) + 1) * N
    gbps = nbytes / (f_ms / 1e3) / 1e9
    line = {"function": name, "values": N, "inputs": len(inputs), "fused_ms": round(f_ms, 3), "fused_ms_min": round(min(tf), 3), "fused_ms_max": round(max(tf), 3),
            "yardstick_ms": round(y_ms, 3), "yardstick_ms_min": round(min(ty), 3), "yardstick_ms_max": round(max(ty), 3),
            "yardstick": "the same formula in torch, float64 math, cast to float32", "speedup": round(y_ms / f_ms, 2), "bytes": nbytes, "gbps": round(gbps, 1),
            "copy_rate_gbps": round(rate / 1e9, 1), "share_of_copy": round(gbps * 1e9 / rate, 4), "allclose_to_yardstick": same, "max_rel_difference": worst,
            "not_slower": bool(f_ms <= y_ms + spread), "spread_ms": round(spread, 3), "reps": args.reps}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del inputs
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
