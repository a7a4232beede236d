"""The seven OI calls of profiles/oi_union_selection_ab.txt with the library GPP_LIB names (default: the tree's): per call one JSON line
with the SHA-256 of the float32 output bytes (equal digests <=> np.array_equal, NaN payloads included), ms per call (three blocking calls
behind one warm-up, each call synchronised) and the pair-table statistics.  Two libraries are compared by running this once per library in
one session and comparing the lines.  usage: oi_pair_table_cases.py [case ...]   (cases: smooth var mp20 mp40 mp50 spatial headline)"""
import hashlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import gridpp_amd as gridpp
from tools.bench_cases import make_workload, oi_inputs


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype=np.float32).tobytes())
    return h.hexdigest()


def run(name, call):
    call(); torch.cuda.synchronize()
    first = gridpp.oi_last_stats()
    ms = []
    for _ in range(3):
        t0 = time.perf_counter(); out = call(); torch.cuda.synchronize(); ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    s = gridpp.oi_last_stats()
    outs = out if isinstance(out, tuple) else (out,)
    print(json.dumps({"case": name, "sha256": digest(*outs), "ms": ms, "solves": s["solves"], "declined_tiles": s["fallback_tiles"],
                      "pair_window": s.get("pair_window", 0), "pair_table_bytes": s.get("pair_table_bytes", 0),
                      "pair_fallback_items": s.get("pair_fallback_items", 0), "pair_table_build_ms": round(first.get("pair_table_build_ms", 0.0), 3)}), flush=True)


def plain(ny, S, mp, var=False, elev=False):
    lats, lons, bg, plat, plon, obs, ratios, pbg, ge, gl, pe, pl, v, w = oi_inputs(ny, ny, S, 1002, elev)
    grid, points, st = gridpp.Grid(lats, lons, ge, gl), gridpp.Points(plat, plon, pe, pl), gridpp.BarnesStructure(10000, v, w)
    d = [torch.from_numpy(a).cuda() for a in (bg, obs, ratios, pbg)]
    if not var:
        return lambda: gridpp.optimal_interpolation(grid, d[0], points, d[1], d[2], d[3], st, mp)
    bv, bvp = torch.ones((ny, ny), dtype=torch.float32, device="cuda"), torch.ones(S, dtype=torch.float32, device="cuda")
    return lambda: gridpp.optimal_interpolation_full(grid, d[0], bv, points, d[1], d[2], d[3], bvp, st, mp)


def spatial(ny, S):
    lats, lons, bg, plat, plon, obs, ratios, pbg = make_workload(ny, ny, S, 1002, 0, ny)
    grid, points = gridpp.Grid(lats, lons), gridpp.Points(plat, plon)
    d = [torch.from_numpy(a).cuda() for a in (bg, obs, ratios, pbg)]
    h = (10000 * np.random.default_rng(3).uniform(0.8, 1.2, (ny, ny))).astype(np.float32)
    z = np.zeros((ny, ny), np.float32)
    st = gridpp.BarnesStructure(grid, h, z, z)
    return lambda: gridpp.optimal_interpolation(grid, d[0], points, d[1], d[2], d[3], st, 30)


CASES = {
    "smooth": ("smooth terrain 2000 x 2000, 2 500 obs, mp 30", lambda: plain(2000, 2500, 30, elev=True)),
    "var": ("2000 x 2000, 2 500 obs, mp 30, with a variance", lambda: plain(2000, 2500, 30, var=True)),
    "mp20": ("1000 x 1000, 625 obs, max_points 20", lambda: plain(1000, 625, 20)),
    "mp40": ("2000 x 2000, 2 500 obs, max_points 40 (48-column form)", lambda: plain(2000, 2500, 40)),
    "mp50": ("2000 x 2000, 2 500 obs, max_points 50 (64-column form)", lambda: plain(2000, 2500, 50)),
    "spatial": ("spatially varying Barnes 2000 x 2000, 2 500 obs, mp 30", lambda: spatial(2000, 2500)),
    "headline": ("the headline call 4000 x 4000, 10 000 obs, mp 30", lambda: plain(4000, 10000, 30)),
}
for key in (sys.argv[1:] or list(CASES)):
    name, make = CASES[key]
    run(name, make())
