"""The cube-layout gradients and the planned ensemble downscalers of a DownscalingPlan against what a user writes without them,
fields resident in HBM (a sibling of tools/bench_downscale_plan.py: the same geometries, timing and spread reporting).

    python tools/bench_downscale_plan_cube.py [--parent-tree DIR] [--in 1000 --out 4000 --members 50] [--jsonl FILE] [--run LABEL]

One JSON line per measurement, then one comparison line per new method and a summary line.  Every time is a host clock around a call
that ends in a device synchronise; every sample of the timed window is kept: median, min and max are reported, the spread of a
measurement is max - min.

  baseline       the chain a user writes today for an ensemble cube (Y, X, E): permute -> contiguous -> plan.full_gradient /
                 plan.simple_gradient on (E, Y, X), a shared gradient broadcast to E levels -> permute -> contiguous; and the direct
                 downscale_probability / mask_threshold_downscale_quantile, which search on every call.  With --parent-tree (a
                 checkout of the parent commit, its library built) they are measured on THAT package and library, in a child process
                 of its own that ends before this one opens the GPU; without, on this build.
  cube methods   plan.full_gradient_cube with shared (Y, X) gradients and with per-member (Y, X, E) gradients,
                 plan.simple_gradient_cube, and beside them plan.apply_cube of the same build: the floor of their loads
  planned        plan.downscale_probability and plan.mask_threshold_downscale_quantile (Nearest plan)
  comparison     new against baseline: the gap of the medians against the larger of the two spreads
Every new result is compared with its baseline of this build bit for bit before anything is timed."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_downscale_plan import Log, samples, summary   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--in", dest="nin", type=int, default=1000, help="the input grid is IN x IN")
    ap.add_argument("--out", dest="nout", type=int, default=4000, help="the output grid is OUT x OUT")
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--jsonl", help="append every line to this file as well")
    ap.add_argument("--run", help="a label added to every line")
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built: the baselines are measured on it, in a child process")
    ap.add_argument("--only-baseline", action="store_true", help="measure the baselines alone (what the child process runs)")
    ap.add_argument("--tree", default=ROOT, help="the checkout to import gridpp_amd from (the child process: the parent's)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    log = Log(None if args.only_baseline else args.jsonl, args.run)
    geometry = "%d^2 -> %d^2" % (args.nin, args.nout)

    parent = None
    if args.parent_tree and not args.only_baseline:
        env = {k: v for k, v in os.environ.items() if k != "GPP_LIB"}
        cmd = [sys.executable, os.path.abspath(__file__), "--only-baseline", "--tree", os.path.abspath(args.parent_tree), "--in", str(args.nin),
               "--out", str(args.nout), "--members", str(args.members), "--reps", str(args.reps)]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            sys.exit("the baselines on the parent build failed:\n" + out.stdout + out.stderr)
        parent = {}
        for line in out.stdout.splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                parent[rec["name"]] = rec
                log(dict(rec, name=rec["name"] + "_parent_build"))

    import numpy as np
    import torch
    import gridpp_amd as gridpp
    from gridpp_amd import _capi
    if gridpp.device_count() < 1:
        sys.exit("no HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    ni, no, E, reps = args.nin, args.nout, args.members, args.reps
    rng = np.random.default_rng(1002)
    lats, lons = np.meshgrid(np.linspace(55.0, 65.0, ni), np.linspace(5.0, 15.0, ni), indexing="ij")
    olats, olons = np.meshgrid(np.linspace(55.01, 64.99, no), np.linspace(5.01, 14.99, no), indexing="ij")
    igrid = gridpp.Grid(lats, lons, rng.uniform(0, 2000, (ni, ni)).astype(np.float32), rng.uniform(0, 1, (ni, ni)).astype(np.float32))
    ogrid = gridpp.Grid(olats, olons, rng.uniform(0, 2000, (no, no)).astype(np.float32), rng.uniform(0, 1, (no, no)).astype(np.float32))
    del lats, lons, olats, olons
    gen = torch.Generator(device=dev).manual_seed(7)
    cube = torch.randn((ni, ni, E), generator=gen, device=dev)
    egrad = torch.randn((ni, ni), generator=gen, device=dev) * 0.002 - 0.0065
    lgrad = torch.randn((ni, ni), generator=gen, device=dev) + 2
    ecube = torch.randn((ni, ni, E), generator=gen, device=dev) * 0.002 - 0.0065
    lcube = torch.randn((ni, ni, E), generator=gen, device=dev) + 2
    threshold = torch.randn((no, no), generator=gen, device=dev)
    nG, nq = ni * ni, no * no
    bil, near = gridpp.downscaling_plan(igrid, ogrid, gridpp.Bilinear), gridpp.downscaling_plan(igrid, ogrid, gridpp.Nearest)

    def to_levels(c):
        return c.permute(2, 0, 1).contiguous() if c.dim() == 3 else c.expand(E, ni, ni).contiguous()

    def chain_full(eg, lg):
        """what a user writes without full_gradient_cube: through the (T, Y, X) layout and back, a shared gradient broadcast"""
        return bil.full_gradient(to_levels(cube), to_levels(eg), to_levels(lg)).permute(1, 2, 0).contiguous()

    baseline = {
        "full_gradient_shared": lambda: chain_full(egrad, lgrad),
        "full_gradient_per_member": lambda: chain_full(ecube, lcube),
        "simple_gradient": lambda: bil.simple_gradient(to_levels(cube), -0.0065).permute(1, 2, 0).contiguous(),
        "downscale_probability": lambda: gridpp.downscale_probability(igrid, ogrid, cube, threshold, gridpp.Gt),
        "mask_threshold_downscale_quantile": lambda: gridpp.mask_threshold_downscale_quantile(igrid, ogrid, cube, ecube, lcube, threshold, gridpp.Gt, 0.5),
    }
    here = {}
    for name, fn in baseline.items():
        here[name] = log(summary("baseline_" + name, samples(fn, 2, reps), geometry=geometry, members=E, library=_capi.LIB_PATH))
    if args.only_baseline:
        return
    ref = {k: (parent["baseline_" + k] if parent is not None else v) for k, v in here.items()}

    new = {
        "full_gradient_shared": lambda: bil.full_gradient_cube(cube, egrad, lgrad),
        "full_gradient_per_member": lambda: bil.full_gradient_cube(cube, ecube, lcube),
        "simple_gradient": lambda: bil.simple_gradient_cube(cube, -0.0065),
        "downscale_probability": lambda: near.downscale_probability(cube, threshold, gridpp.Gt),
        "mask_threshold_downscale_quantile": lambda: near.mask_threshold_downscale_quantile(cube, ecube, lcube, threshold, gridpp.Gt, 0.5),
    }
    for name, fn in new.items():
        a, b = fn(), baseline[name]()
        equal = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)) or torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)))
        log(dict(name="parity_" + name, geometry=geometry, bit_equal=equal))
        if not equal:
            sys.exit("%s differs from its baseline" % name)
        del a, b

    floor = log(summary("apply_cube", samples(lambda: bil.apply_cube(cube), 2, reps), geometry=geometry, members=E))
    wins = []
    for name, fn in new.items():
        t = log(summary("new_" + name, samples(fn, 2, reps), geometry=geometry, members=E))
        d = ref[name]
        gap = d["ms_median"] - t["ms_median"]
        spread = max(d["spread_ms"], t["spread_ms"])
        wins.append(bool(gap > spread))
        rec = dict(name="compare_" + name, geometry=geometry, baseline_from="parent build" if parent is not None else "this build",
                   baseline_ms=d["ms_median"], baseline_this_build_ms=here[name]["ms_median"], new_ms=t["ms_median"], gap_ms=gap,
                   larger_spread_ms=spread, new_wins_by_more_than_the_spread=wins[-1], speedup=d["ms_median"] / t["ms_median"])
        if "gradient" in name:
            rec.update(apply_cube_ms=floor["ms_median"], over_apply_cube=t["ms_median"] / floor["ms_median"])
        log(rec)
    log(dict(name="summary", geometry=geometry, every_new_method_wins=all(wins)))


if __name__ == "__main__":
    main()
