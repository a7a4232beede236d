"""neighbourhood_members and calc_gradient_members against what a user writes without them, cubes resident in HBM (a sibling
of tools/bench_downscale_plan_cube.py: the same timing and spread reporting).

    python tools/bench_members.py [--sizes 1000 4000] [--members 50] [--parent-tree DIR] [--jsonl FILE] [--run LABEL] [--ab]

One JSON line per measurement, one comparison line per case and a summary line per geometry.  Every time is a host clock around a call that
ends in a device synchronise; every sample of the timed window is kept: median, min and max are reported, the spread of a measurement is
max - min.

  chain        what a user writes today for a cube (Y, X, E): cube.permute(2, 0, 1).contiguous(), E direct calls of neighbourhood(plane, ...)
               or calc_gradient(base, plane, ...), torch.stack(planes, -1).  With --parent-tree (a checkout of the parent commit, its library
               built) it is measured on THAT package and library as well, in a child process of its own that ends before this one opens the GPU.
  new          neighbourhood_members(cube, ...) / calc_gradient_members(base, cube, ...)
  copy         out.copy_(cube): the cube read once and written once, the traffic the algorithm cannot avoid
  comparison   new against chain: the gap of the medians against the larger of the two spreads; the algorithmic floor 2 Y X E 4 B (+ Y X 4 B
               for a shared base) over the new call's median as GB/s, and that time as a multiple of the copy's
Every new result is compared with its chain bit for bit on exact data (tests/members_ref.py: multiples of 1/8, 3 % missing), with and without
missing values, before anything is timed; the timed cubes are the ones without missing values.
--ab: the neighbourhood cases once more with the two-pass form forced (GPP_MEMBERS_TWO_PASS) where the fused form is the default."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_downscale_plan import Log, samples, summary   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("Mean", 1), ("Mean", 7), ("Mean", 15), ("Max", 7), ("Variance", 7), ("MinMax", 5), ("LinearRegression", 5)]


def case_name(stat, hw):
    return "%s_hw%d" % (stat, hw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4000], help="the cubes are N x N x members")
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--jsonl", help="append every line to this file as well")
    ap.add_argument("--run", help="a label added to every line")
    ap.add_argument("--ab", action="store_true", help="also time the neighbourhood cases with the two-pass form forced")
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built: the chains are measured on it too, in a child process")
    ap.add_argument("--only-chain", action="store_true", help="measure the chains alone (what the child process runs)")
    ap.add_argument("--tree", default=ROOT, help="the checkout to import gridpp_amd from (the child process: the parent's)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    log = Log(None if args.only_chain else args.jsonl, args.run)

    parent = None
    if args.parent_tree and not args.only_chain:
        env = {k: v for k, v in os.environ.items() if k != "GPP_LIB"}
        cmd = [sys.executable, os.path.abspath(__file__), "--only-chain", "--tree", os.path.abspath(args.parent_tree), "--members", str(args.members),
               "--reps", str(args.reps), "--sizes"] + [str(n) for n in args.sizes]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1100)
        if out.returncode != 0:
            sys.exit("the chains on the parent build failed:\n" + out.stdout + out.stderr)
        parent = {}
        for line in out.stdout.splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                parent[(rec["name"], rec["geometry"])] = rec
                log(dict(rec, name=rec["name"] + "_parent_build"))

    import torch
    import gridpp_amd as gridpp
    from gridpp_amd import _capi
    if gridpp.device_count() < 1:
        sys.exit("no HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    E, reps = args.members, args.reps

    for n in args.sizes:
        geometry = "%d^2 x %d" % (n, E)
        gen = torch.Generator(device=dev).manual_seed(7 + n)
        # exact data: multiples of 1/8 with |v| <= 64 (every sum exact in double, every product exact in float32)
        cube = torch.randint(-512, 513, (n, n, E), generator=gen, device=dev).to(torch.float32) / 8
        base = torch.randint(-512, 513, (n, n), generator=gen, device=dev).to(torch.float32) / 8
        holes = cube.clone()
        holes[torch.rand((n, n, E), generator=gen, device=dev) < 0.03] = float("nan")
        holes[n // 3:n // 3 + 40, n // 4:n // 4 + 60, :] = float("nan")
        hbase = base.clone()
        hbase[torch.rand((n, n), generator=gen, device=dev) < 0.03] = float("nan")

        def chain(stat, hw, c=cube, b=base):
            planes = c.permute(2, 0, 1).contiguous()
            if stat in ("MinMax", "LinearRegression"):
                out = [gridpp.calc_gradient(b, planes[e], getattr(gridpp, stat), hw) for e in range(E)]
            else:
                out = [gridpp.neighbourhood(planes[e], hw, getattr(gridpp, stat)) for e in range(E)]
            return torch.stack(out, -1)

        def new(stat, hw, c=cube, b=base):
            if stat in ("MinMax", "LinearRegression"):
                return gridpp.calc_gradient_members(b, c, getattr(gridpp, stat), hw)
            return gridpp.neighbourhood_members(c, hw, getattr(gridpp, stat))

        here = {}
        for stat, hw in CASES:
            name = case_name(stat, hw)
            here[name] = log(summary("chain_" + name, samples(lambda: chain(stat, hw), 2, reps), geometry=geometry, library=os.path.relpath(_capi.LIB_PATH, os.path.abspath(args.tree))))
        if args.only_chain:
            continue

        for stat, hw in CASES:
            for label, c, b in (("complete", cube, base), ("missing", holes, hbase)):
                a, w = new(stat, hw, c, b), chain(stat, hw, c, b)
                equal = bool(torch.equal(a.view(torch.int32), w.view(torch.int32)) or
                             (torch.equal(torch.isnan(a), torch.isnan(w)) and torch.equal(torch.nan_to_num(a, nan=0.0).view(torch.int32), torch.nan_to_num(w, nan=0.0).view(torch.int32))))
                log(dict(name="parity_" + case_name(stat, hw), geometry=geometry, data=label, bit_equal=equal))
                if not equal:
                    sys.exit("%s differs from its chain on %s data" % (case_name(stat, hw), label))
                del a, w

        out = torch.empty_like(cube)
        copy = log(summary("copy", samples(lambda: out.copy_(cube), 2, reps), geometry=geometry))
        del out
        wins = []
        for stat, hw in CASES:
            name = case_name(stat, hw)
            t = log(summary("new_" + name, samples(lambda: new(stat, hw), 2, reps), geometry=geometry))
            d = here[name]
            gap = d["ms_median"] - t["ms_median"]
            spread = max(d["spread_ms"], t["spread_ms"])
            wins.append(bool(gap > spread))
            floor_bytes = 2 * n * n * E * 4 + (n * n * 4 if stat in ("MinMax", "LinearRegression") else 0)
            rec = dict(name="compare_" + name, geometry=geometry, chain_ms=d["ms_median"], new_ms=t["ms_median"], gap_ms=gap, larger_spread_ms=spread,
                       new_wins_by_more_than_the_spread=wins[-1], speedup=d["ms_median"] / t["ms_median"], floor_bytes=floor_bytes,
                       floor_gb_per_s=floor_bytes / (t["ms_median"] * 1e-3) / 1e9, copy_ms=copy["ms_median"], over_copy=t["ms_median"] / copy["ms_median"])
            if parent is not None:
                rec.update(chain_parent_build_ms=parent[("chain_" + name, geometry)]["ms_median"])
            log(rec)
        log(dict(name="summary", geometry=geometry, every_new_call_wins=all(wins)))

        if args.ab:
            gridpp.set_path_override("GPP_MEMBERS_TWO_PASS", 1)
            try:
                for stat, hw in CASES[:5]:
                    log(summary("ab_two_pass_" + case_name(stat, hw), samples(lambda: new(stat, hw), 2, reps), geometry=geometry))
            finally:
                gridpp.set_path_override("GPP_MEMBERS_TWO_PASS", None)
        del cube, base, holes, hbase
        gridpp.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
