"""The reusable downscaling plan against the direct calls it replaces, fields resident in HBM.

    python tools/bench_downscale_plan.py [--parent-tree DIR] [--in 1000 --out 4000 --levels 24 --members 50] [--jsonl FILE] [--run LABEL]

One JSON line per measurement, then one comparison line per planned method and a summary line.  Every time is a host clock around a call
that ends in a device synchronise (the entry points synchronise the library stream before they return); every sample of the timed
window is kept: median, min and max are reported, the spread of a measurement is max - min.

  direct calls   bilinear / nearest at T = 1 and T = levels, full_gradient (Bilinear) at T = levels, and for the ensemble cube the
                 chain a user writes without apply_cube: permute -> contiguous -> bilinear -> permute -> contiguous in torch.  With
                 --parent-tree (a checkout of the parent commit, its library built) they are measured on THAT package and library,
                 in a child process of its own that ends before this one opens the GPU; without, on this build.
  t_build        downscaling_plan (nearest-neighbour search, boxes and weights, the copies of the elevations and lafs; allocation
                 of the records included), Bilinear and Nearest
  planned calls  plan.apply at T = 1 and T = levels (both downscalers), plan.full_gradient at T = levels, plan.apply_cube at E = members
  comparison     planned against direct: the gap of the medians against the larger of the two spreads, and the break-even number of
                 calls t_build / (t_direct - t_planned)
  bytes          distinct bytes of a planned call (every input value once, the records, the output) over its time, as a share of
                 8 TB/s; for apply_cube also the requested bytes (4 corners + 1 nearest + 1 output) * 4 E per location.
The planned results are compared with the direct ones of this build bit for bit before anything is timed."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBS = 8.0


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


class Log:
    def __init__(self, path, run=None):
        self.path, self.run = path, run

    def __call__(self, rec):
        line = json.dumps(rec if self.run is None else dict(rec, run=self.run))
        print(line, flush=True)
        if self.path:
            with open(self.path, "a") as f:
                f.write(line + "\n")
        return rec


def summary(name, ts, **extra):
    return dict(name=name, ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), spread_ms=max(ts) - min(ts), samples=len(ts), **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--in", dest="nin", type=int, default=1000, help="the input grid is IN x IN")
    ap.add_argument("--out", dest="nout", type=int, default=4000, help="the output grid is OUT x OUT")
    ap.add_argument("--levels", type=int, default=24)
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--jsonl", help="append every line to this file as well")
    ap.add_argument("--run", help="a label added to every line (to tell a repeated run from the first in one file)")
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built: the direct calls are measured on it, in a child process")
    ap.add_argument("--only-direct", action="store_true", help="measure the direct calls alone (what the child process runs)")
    ap.add_argument("--tree", default=ROOT, help="the checkout to import gridpp_amd from (the child process: the parent's)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    log = Log(None if args.only_direct else args.jsonl, args.run)
    geometry = "%d^2 -> %d^2" % (args.nin, args.nout)

    parent = None
    if args.parent_tree and not args.only_direct:
        env = {k: v for k, v in os.environ.items() if k != "GPP_LIB"}
        cmd = [sys.executable, os.path.abspath(__file__), "--only-direct", "--tree", os.path.abspath(args.parent_tree), "--in", str(args.nin),
               "--out", str(args.nout), "--levels", str(args.levels), "--members", str(args.members), "--reps", str(args.reps)]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            sys.exit("the direct calls on the parent build failed:\n" + out.stdout + out.stderr)
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
    ni, no, T, E, reps = args.nin, args.nout, args.levels, args.members, args.reps
    rng = np.random.default_rng(1002)
    lats, lons = np.meshgrid(np.linspace(55.0, 65.0, ni), np.linspace(5.0, 15.0, ni), indexing="ij")
    olats, olons = np.meshgrid(np.linspace(55.01, 64.99, no), np.linspace(5.01, 14.99, no), indexing="ij")
    igrid = gridpp.Grid(lats, lons, rng.uniform(0, 2000, (ni, ni)).astype(np.float32), rng.uniform(0, 1, (ni, ni)).astype(np.float32))
    ogrid = gridpp.Grid(olats, olons, rng.uniform(0, 2000, (no, no)).astype(np.float32), rng.uniform(0, 1, (no, no)).astype(np.float32))
    del lats, lons, olats, olons
    gen = torch.Generator(device=dev).manual_seed(7)
    values = torch.randn((T, ni, ni), generator=gen, device=dev)
    egrad = torch.randn((T, ni, ni), generator=gen, device=dev) * 0.002 - 0.0065
    lgrad = torch.randn((T, ni, ni), generator=gen, device=dev) + 2
    cube = torch.randn((ni, ni, E), generator=gen, device=dev)
    one = values[:1].contiguous()
    nG, nq = ni * ni, no * no

    def direct_cube(c):
        """what a user writes without apply_cube: the cube through bilinear's (T, Y, X) layout and back"""
        return gridpp.bilinear(igrid, ogrid, c.permute(2, 0, 1).contiguous()).permute(1, 2, 0).contiguous()

    direct = {
        "bilinear_T1": lambda: gridpp.bilinear(igrid, ogrid, one),
        "bilinear_T%d" % T: lambda: gridpp.bilinear(igrid, ogrid, values),
        "nearest_T1": lambda: gridpp.nearest(igrid, ogrid, one),
        "nearest_T%d" % T: lambda: gridpp.nearest(igrid, ogrid, values),
        "full_gradient_T%d" % T: lambda: gridpp.full_gradient(igrid, ogrid, values, egrad, lgrad, gridpp.Bilinear),
        "cube_E%d" % E: lambda: direct_cube(cube),
    }
    here = {}
    for name, fn in direct.items():
        few = name.endswith("T%d" % T) or name.startswith("cube")
        here[name] = log(summary("direct_" + name, samples(fn, 2, max(3, reps // 2) if few else reps), geometry=geometry, library=_capi.LIB_PATH))
    if args.only_direct:
        return
    ref = {k: (parent["direct_" + k] if parent is not None else v) for k, v in here.items()}

    holder = {}

    def build(ds):
        holder.pop(ds, None)          # (the records of the previous plan go back first: a build allocates its own)
        holder[ds] = gridpp.downscaling_plan(igrid, ogrid, ds)
    t_build = {}
    for ds, label in ((gridpp.Bilinear, "bilinear"), (gridpp.Nearest, "nearest")):
        t_build[label] = log(summary("t_build_" + label, samples(lambda: build(ds), 1, 5), geometry=geometry))
    bil, near = holder[gridpp.Bilinear], holder[gridpp.Nearest]
    log(dict(name="plan_info", geometry=geometry, nbytes_bilinear=bil.nbytes, nbytes_nearest=near.nbytes, distorted=bil.distorted))

    planned = {
        "bilinear_T1": (lambda: bil.apply(one), "bilinear", 16 * nq + 4 * nG + 4 * nq),
        "bilinear_T%d" % T: (lambda: bil.apply(values), "bilinear", 16 * nq + T * 4 * (nG + nq)),
        "nearest_T1": (lambda: near.apply(one), "nearest", 4 * nq + 4 * nG + 4 * nq),
        "nearest_T%d" % T: (lambda: near.apply(values), "nearest", 4 * nq + T * 4 * (nG + nq)),
        "full_gradient_T%d" % T: (lambda: bil.full_gradient(values, egrad, lgrad), "bilinear", 16 * nq + 8 * nG + 8 * nq + T * 4 * (3 * nG + nq)),
        "cube_E%d" % E: (lambda: bil.apply_cube(cube), "bilinear", 16 * nq + 4 * E * (nG + nq)),
    }
    # the planned results are the direct ones of this build, bit for bit
    for name, (fn, _, _) in planned.items():
        a, b = fn(), direct[name]()
        equal = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)) or torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)))
        log(dict(name="parity_" + name, geometry=geometry, bit_equal=equal))
        if not equal:
            sys.exit("planned %s differs from the direct call" % name)
        del a, b

    wins = []
    for name, (fn, label, distinct) in planned.items():
        few = name.endswith("T%d" % T) or name.startswith("cube")
        extra = dict(geometry=geometry, distinct_bytes=distinct)
        if name.startswith("cube"):
            extra["requested_bytes"] = 6 * 4 * E * nq + 16 * nq
        t = summary("planned_" + name, samples(fn, 2, max(3, reps // 2) if few else reps), **extra)
        sec = t["ms_median"] * 1e-3
        t["distinct_TBps"] = distinct / sec / 1e12
        t["share_of_%g_TBps" % HBM_TBS] = t["distinct_TBps"] / HBM_TBS
        if "requested_bytes" in extra:
            t["requested_TBps"] = extra["requested_bytes"] / sec / 1e12
        log(t)
        d = ref[name]
        gap = d["ms_median"] - t["ms_median"]
        spread = max(d["spread_ms"], t["spread_ms"])
        wins.append(bool(gap > spread))
        log(dict(name="compare_" + name, geometry=geometry, direct_from="parent build" if parent is not None else "this build",
                 direct_ms=d["ms_median"], direct_this_build_ms=here[name]["ms_median"], planned_ms=t["ms_median"], gap_ms=gap, larger_spread_ms=spread,
                 planned_wins_by_more_than_the_spread=wins[-1], speedup=d["ms_median"] / t["ms_median"], t_build_ms=t_build[label]["ms_median"],
                 break_even_calls=(t_build[label]["ms_median"] / gap if gap > 0 else None)))
    log(dict(name="summary", geometry=geometry, every_planned_method_wins=all(wins)))


if __name__ == "__main__":
    main()
