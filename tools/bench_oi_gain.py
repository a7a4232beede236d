"""The reusable OI gain on the headline geometry (4000 x 4000 grid, 10 000 stations, BarnesStructure(10000), max_points 30, fields
resident in HBM): what a loop of E optimal_interpolation calls costs against one gain and one apply of an E-field stack.

    python tools/bench_oi_gain.py [--parent-tree DIR] [--ny 4000 --nx 4000 --obs 10000 --max-points 30 --fields 50]

One JSON line per measurement, then a summary line.  Every time is a host clock around a call that ends in a device synchronise (the
entry points synchronise the library stream before they return); every sample of the timed window is kept: median, min and max are
reported, the spread of a measurement is max - min.

  t_oi        one optimal_interpolation call.  With --parent-tree (a checkout of the parent commit, its library built) it is measured on
              THAT package and library, in a child process of its own that runs before this one opens the GPU; without, on this build.
  t_build     optimal_interpolation_gain (scan, one inversion per distinct selection of a tile, weights; allocation of the planes included)
  t_apply_1   gain.apply of one field
  t_apply_E   gain.apply of a stack of E fields, one call
  condition   t_build + t_apply_E < E * t_oi, and the gap against the larger of the two spreads (E * spread(t_oi) on the right-hand side)
  break_even  E* = t_build / (t_oi - t_apply_1)
  bytes/s     the algorithmic floor of an apply, cells * K * 12 B + cells * E * 8 B, over its time (the innovation table stays in L2);
              K is max_points.  Beside it: 5.8 TB/s, what k_member_pass streams on the same chip.
The one-field apply is also compared with optimal_interpolation on the same inputs (the measure of the suite)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_YARDSTICK_TBS = 5.8


def samples(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def summary(name, ts, **extra):
    rec = dict(name=name, ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), spread_ms=max(ts) - min(ts), samples=len(ts), **extra)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, default=4000)
    ap.add_argument("--nx", type=int, default=4000)
    ap.add_argument("--obs", type=int, default=10000)
    ap.add_argument("--max-points", type=int, default=30)
    ap.add_argument("--h", type=float, default=10000.0)
    ap.add_argument("--fields", type=int, default=50)
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built: t_oi is measured on it, in a child process")
    ap.add_argument("--only-oi", action="store_true", help="measure t_oi alone (what the child process runs)")
    ap.add_argument("--tree", default=ROOT, help="the checkout to import gridpp_amd from (the child process: the parent's)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))

    parent = None
    if args.parent_tree and not args.only_oi:
        env = {k: v for k, v in os.environ.items() if k != "GPP_LIB"}
        cmd = [sys.executable, os.path.abspath(__file__), "--only-oi", "--tree", os.path.abspath(args.parent_tree), "--ny", str(args.ny), "--nx", str(args.nx), "--obs", str(args.obs),
               "--max-points", str(args.max_points), "--h", str(args.h)]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            sys.exit("t_oi on the parent build failed:\n" + out.stdout + out.stderr)
        parent = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        parent["name"] = "t_oi_parent_build"
        print(json.dumps(parent), flush=True)

    import numpy as np
    import torch
    import gridpp_amd as gridpp
    from gridpp_amd import _capi
    from tools.bench_cases import make_workload
    if gridpp.device_count() < 1:
        sys.exit("no HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    ny, nx, S, K, E = args.ny, args.nx, args.obs, args.max_points, args.fields
    lats, lons, bg, plat, plon, obs, ratios, pbg = make_workload(ny, nx, S, 1002, 0, ny)
    grid, points, structure = gridpp.Grid(lats, lons), gridpp.Points(plat, plon), gridpp.BarnesStructure(args.h)
    d_bg, d_obs, d_ratios, d_pbg = (torch.from_numpy(a).to(dev) for a in (bg, obs, ratios, pbg))
    cells = ny * nx

    oi = lambda: gridpp.optimal_interpolation(grid, d_bg, points, d_obs, d_ratios, d_pbg, structure, K)
    t_oi = summary("t_oi", samples(oi, 3, 10), library=_capi.LIB_PATH, cells=cells, stations=S, max_points=K)
    if args.only_oi:
        return
    ref_oi = t_oi if parent is None else parent

    holder = []

    def build():
        holder.clear()          # (the planes of the previous gain go back first: a build allocates its own)
        holder.append(gridpp.optimal_interpolation_gain(grid, points, ratios, structure, K))
    t_build = summary("t_build", samples(build, 1, 3))
    gain = holder[0]
    nbytes = gain.nbytes
    out1 = gain.apply(d_bg, d_obs, d_pbg)
    ref = oi()
    err = float(torch.max(torch.abs(out1.double() - ref.double()) / torch.clamp(torch.abs(ref.double()), min=1e-3)))
    print(json.dumps(dict(name="apply_1_vs_optimal_interpolation", max_rel_err=err, nbytes=nbytes, largest_selection=gain.largest_selection)), flush=True)
    del ref

    def floor(e):
        return cells * K * 12 + cells * e * 8
    t_a1 = summary("t_apply_1", samples(lambda: gain.apply(d_bg, d_obs, d_pbg), 2, 10), floor_bytes=floor(1))
    rng = np.random.default_rng(7)
    d_stack = d_bg[..., None] + torch.from_numpy(rng.normal(0, 0.5, E).astype(np.float32)).to(dev)          # (Y, X, E)
    d_pbgs = d_pbg[:, None] + torch.from_numpy(rng.normal(0, 0.5, (S, E)).astype(np.float32)).to(dev)       # (S, E)
    d_stack, d_pbgs = d_stack.contiguous(), d_pbgs.contiguous()
    t_ae = summary("t_apply_%d" % E, samples(lambda: gain.apply(d_stack, d_obs, d_pbgs), 1, 5), floor_bytes=floor(E), fields=E)

    lhs = t_build["ms_median"] + t_ae["ms_median"]
    rhs = E * ref_oi["ms_median"]
    spread = max(t_build["spread_ms"] + t_ae["spread_ms"], E * ref_oi["spread_ms"])
    denom = ref_oi["ms_median"] - t_a1["ms_median"]
    print(json.dumps(dict(
        name="summary", fields=E, t_oi_from="parent build" if parent is not None else "this build",
        t_oi_ms=ref_oi["ms_median"], t_oi_this_build_ms=t_oi["ms_median"], t_build_ms=t_build["ms_median"], t_apply_1_ms=t_a1["ms_median"],
        t_apply_E_ms=t_ae["ms_median"], build_plus_apply_ms=lhs, loop_of_E_calls_ms=rhs, gap_ms=rhs - lhs, larger_spread_ms=spread,
        condition_holds=bool(lhs < rhs and rhs - lhs > spread), break_even_fields=(t_build["ms_median"] / denom if denom > 0 else None),
        apply_1_TBps=floor(1) / (t_a1["ms_median"] * 1e-3) / 1e12, apply_E_TBps=floor(E) / (t_ae["ms_median"] * 1e-3) / 1e12,
        streaming_yardstick_TBps=STREAM_YARDSTICK_TBS, gain_nbytes=nbytes)), flush=True)


if __name__ == "__main__":
    main()
