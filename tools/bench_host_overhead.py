"""Host overhead of an entry point: the per-call wall time of six tiny device-resident calls where everything is overhead, this tree against
a checkout of the parent commit (the launch helper adds one hipGetLastError per launch on the good path).

    python tools/bench_host_overhead.py --parent-tree DIR [--rounds 5] [--calls 2000] [--jsonl FILE]

  calc_crps      64 rows x 8 members       (one launch)
  neighbourhood  Mean, halfwidth 1, 16 x 16 (one launch)
  fill_missing   16 x 16                    (five launches)
  oi             optimal_interpolation, 16 x 16 grid, 8 observations, max_points 4 (the OiCall path: pack, tile kernel, list passes)
  oi_ensi        optimal_interpolation_ensi on the same geometry, 4 members         (the EnsiCall path: scan, pair, members)
  oi_gain_apply  OiGain.apply with one field, the gain built once on that geometry  (two launches)

Each is timed twice: `abi` is the extern "C" entry called through ctypes with device pointers and a preallocated result, `api` the Python wrapper a
user calls.  A call ends in the library's own stream synchronise, so the host clock around it is the whole call.  A measurement is a warm-up of 200
calls, then the median of --calls calls.  Every measurement runs in a child process of its own that ends before the next starts (this process never
opens the GPU): a discarded first process, then --rounds rounds that alternate the parent's tree and this one.  One JSON line per child, then one
comparison line per call: the medians of both trees per round, the round-to-round spread (max - min of the medians) of each tree, and whether the
median over this tree's rounds lies within the larger spread of the parent's median.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(tree, calls):
    sys.path.insert(0, os.path.abspath(tree))
    import ctypes as C
    import numpy as np
    import torch
    import gridpp_amd as gridpp
    from gridpp_amd import _capi
    if gridpp.device_count() < 1:
        sys.exit("no HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(11)
    ens = torch.rand((64, 8), generator=gen, device=dev)
    ref = torch.rand((64,), generator=gen, device=dev)
    plane = torch.rand((16, 16), generator=gen, device=dev)
    holes = plane.clone()
    holes[3:6, 4:9] = float("nan")
    o64, o256 = torch.empty(64, device=dev), torch.empty((16, 16), device=dev)
    # the OI family: a 16 x 16 grid over one degree, 8 observations inside it, every cell within reach of some of them
    lats, lons = np.meshgrid(np.linspace(60.0, 61.0, 16), np.linspace(10.0, 11.0, 16), indexing="ij")
    rng = np.random.default_rng(11)
    grid, points = gridpp.Grid(lats, lons), gridpp.Points(rng.uniform(60.0, 61.0, 8), rng.uniform(10.0, 11.0, 8))
    structure = gridpp.BarnesStructure(50000)
    pobs, pratios, pbg = (torch.rand((8,), generator=gen, device=dev) for _ in range(3))
    psigmas = pratios + 0.5
    cube, pcube = torch.rand((16, 16, 4), generator=gen, device=dev), torch.rand((8, 4), generator=gen, device=dev)
    ocube = torch.empty((16, 16, 4), device=dev)
    gain = gridpp.optimal_interpolation_gain(grid, points, pratios.cpu().numpy(), structure, 4)
    lib = _capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.byref(structure._s)
    DEVICE = 1   # GPP_MEM_DEVICE
    cases = {
        "calc_crps_abi": lambda: lib.gpp_calc_crps(p(ens), p(ref), 64, 8, p(o64), DEVICE),
        "neighbourhood_abi": lambda: lib.gpp_neighbourhood(p(plane), 16, 16, 1, 0, 1, gridpp.Mean, p(o256), DEVICE),
        "fill_missing_abi": lambda: lib.gpp_fill_missing(p(holes), 16, 16, p(o256), DEVICE),
        "oi_abi": lambda: lib.gpp_optimal_interpolation_full(grid._h, p(plane), None, points._h, p(pobs), p(pratios), p(pbg), None, st, 4, 1, p(o256), None, DEVICE),
        "oi_ensi_abi": lambda: lib.gpp_optimal_interpolation_ensi(grid._h, p(cube), 4, points._h, p(pobs), p(psigmas), p(pcube), st, 4, 1, p(ocube), DEVICE),
        "oi_gain_apply_abi": lambda: lib.gpp_oi_gain_apply(gain._h, p(plane), 1, p(pobs), 0, p(pbg), 1, p(o256), DEVICE),
        "calc_crps_api": lambda: gridpp.calc_crps(ens, ref),
        "neighbourhood_api": lambda: gridpp.neighbourhood(plane, 1, gridpp.Mean),
        "fill_missing_api": lambda: gridpp.fill_missing(holes),
        "oi_api": lambda: gridpp.optimal_interpolation(grid, plane, points, pobs, pratios, pbg, structure, 4),
        "oi_ensi_api": lambda: gridpp.optimal_interpolation_ensi(grid, cube, points, pobs, psigmas, pcube, structure, 4),
        "oi_gain_apply_api": lambda: gain.apply(plane, pobs, pbg),
    }
    out = {}
    for name, fn in cases.items():
        rc = fn()
        if name.endswith("_abi") and rc != 0:
            sys.exit("%s failed: %s" % (name, lib.gpp_last_error()))
        for _ in range(200):
            fn()
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e6)
        ts.sort()
        out[name] = dict(us_median=statistics.median(ts), us_p10=ts[len(ts) // 10], us_p90=ts[9 * len(ts) // 10], us_min=ts[0])
    print(json.dumps(dict(tree=os.path.abspath(tree), library=os.path.relpath(_capi.LIB_PATH, os.path.abspath(tree)), calls=calls, results=out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--jsonl", help="append every line to this file as well")
    ap.add_argument("--only", help="measure this tree alone and print one line (what a child process runs)")
    args = ap.parse_args()
    if args.only:
        return measure(args.only, args.calls)
    if not args.parent_tree:
        sys.exit("--parent-tree is required")

    def log(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.jsonl:
            with open(args.jsonl, "a") as f:
                f.write(line + "\n")

    def child(tree, label):
        env = {k: v for k, v in os.environ.items() if k != "GPP_LIB"}
        cmd = [sys.executable, os.path.abspath(__file__), "--only", os.path.abspath(tree), "--calls", str(args.calls)]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        if out.returncode != 0:
            sys.exit("%s failed:\n%s%s" % (label, out.stdout, out.stderr))
        rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        rec["run"] = label
        del rec["tree"]
        log(rec)
        return rec["results"]

    child(args.parent_tree, "warmup_discarded")
    rounds = {"parent": [], "this": []}
    for r in range(args.rounds):
        order = ("parent", "this") if r % 2 == 0 else ("this", "parent")
        for which in order:
            rounds[which].append(child(args.parent_tree if which == "parent" else ROOT, "%s_r%d" % (which, r + 1)))
    for name in rounds["parent"][0]:
        a = [r[name]["us_median"] for r in rounds["parent"]]
        b = [r[name]["us_median"] for r in rounds["this"]]
        spread = max(max(a) - min(a), max(b) - min(b))
        gap = statistics.median(b) - statistics.median(a)
        log(dict(name="compare_" + name, parent_us=a, this_us=b, parent_spread_us=max(a) - min(a), this_spread_us=max(b) - min(b), larger_spread_us=spread,
                 parent_median_us=statistics.median(a), this_median_us=statistics.median(b), gap_us=gap, within_larger_spread=bool(abs(gap) <= spread),
                 this_rounds_inside_parent_range_plus_spread=sum(min(a) - spread <= x <= max(a) + spread for x in b)))


if __name__ == "__main__":
    main()
