"""A walk over the host branches of optimal_interpolation_ensi and optimal_interpolation_ensi_multi: every branch once, fixed seeds.

    python tools/ensi_host_walk.py run          # the calls; one line per call: sha256 of the output array, or the error message
    python tools/ensi_host_walk.py parse DIR [RUNLOG]   # the ordered kernel dispatches per queue of a traced run (+ the lines of RUNLOG)
on the GPU box, once per library (GPP_LIB selects it), each in a process of its own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/ensi_host_walk.py run > RUNLOG
Two libraries whose `parse` outputs are equal launch the same kernels with the same grids in the same order and return the same bits.
NOT YET RUN on a GPU: only `parse` has been exercised (on a hand-made trace); whether every case reaches the branch its label names, and the
column names of the kernel-trace CSV, are still to be confirmed by the first traced run."""
import csv, glob, hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

F = np.float32


def ensi_case(seed, Y, X, E, S):
    rng = np.random.default_rng(seed)
    lats, lons = np.meshgrid(np.linspace(0, 1, Y), np.linspace(0, 1, X), indexing="ij")
    bg = (np.sin(5 * lats) * np.cos(3 * lons))[:, :, None] + rng.normal(0, 1, (Y, X, E))
    return dict(lats=lats, lons=lons, bg=bg.astype(F), plat=rng.random(S), plon=rng.random(S), pbg=rng.normal(0, 1, (S, E)).astype(F),
                obs=rng.normal(0, 1, S).astype(F), sig=rng.uniform(0.5, 2, S).astype(F),
                gelev=rng.uniform(0, 500, (Y, X)), pelev=rng.uniform(0, 500, S))


def multi_case(seed, variant, n, E, S):
    rng = np.random.default_rng(seed)
    r = lambda *shape: rng.normal(0, 1, shape).astype(F)
    return dict(blat=rng.random(n), blon=rng.random(n), plat=rng.random(S), plon=rng.random(S), bg=r(n, E), bgc=r(n, E), pbg=r(S, E), pbgc=r(S, E),
                pobs=r(S) if variant == "utem" else r(S, E), pr=rng.uniform(0.5, 1.5, S).astype(F), br=rng.uniform(0.5, 1.5, n).astype(F))


def run():
    import gridpp_amd as g
    from contextlib import contextmanager

    @contextmanager
    def switch(name, value):
        g.set_path_override(name, value)
        try:
            yield
        finally:
            g.set_path_override(name, None)

    def report(name, fn):
        try:
            out = np.ascontiguousarray(fn())
            print("%-58s %s %s" % (name, hashlib.sha256(out.tobytes()).hexdigest()[:16], out.shape), flush=True)
        except RuntimeError as e:
            print("%-58s RuntimeError: %s" % (name, e), flush=True)

    def ensi(c, h, mp, allow=True, spatial=False, points_bg=False):
        Y, X, E = c["bg"].shape
        if points_bg:   # the Points overload: the same cells as a point set (no 2-D tiles)
            grid, bg = g.Points(c["lats"].ravel(), c["lons"].ravel()), c["bg"].reshape(-1, E)
        else:
            grid, bg = g.Grid(c["lats"], c["lons"], c["gelev"] if spatial else (), ()), c["bg"]
        points = g.Points(c["plat"], c["plon"], c["pelev"] if spatial else (), ())
        st = g.BarnesStructure(h)
        if spatial:   # scales on a coarser field grid, the structure of the parity tests
            rng = np.random.default_rng(6)
            flat, flon = np.meshgrid(np.linspace(0, 1, 7), np.linspace(0, 1, 9), indexing="ij")
            hf, vf = (h * rng.uniform(0.7, 1.3, flat.shape)).astype(F), (300 * rng.uniform(0.7, 1.3, flat.shape)).astype(F)
            st = g.BarnesStructure(g.Grid(flat, flon), hf, vf, np.zeros(flat.shape, F), 0.0013)
        out = g.optimal_interpolation_ensi(grid, bg, points, c["obs"], c["sig"], c["pbg"], st, mp, allow)
        print("    condition_passthrough %d" % g.ensi_last_stats()["condition_passthrough"])
        return out

    def multi(variant, c, h, mp, allow=True, shape=None):
        if shape:   # the Grid overload: the same numbers on a Y x X grid
            lats, lons = np.meshgrid(np.linspace(0, 1, shape[0]), np.linspace(0, 1, shape[1]), indexing="ij")
            b, rs = g.Grid(lats, lons), lambda a: a.reshape(shape + a.shape[1:])
        else:
            b, rs = g.Points(c["blat"], c["blon"]), lambda a: a
        points, st = g.Points(c["plat"], c["plon"]), g.BarnesStructure(h)
        if variant == "ebesc":
            return g.optimal_interpolation_ensi_multi_ebesc(b, rs(c["br"]), rs(c["bg"]), points, c["pobs"], c["pr"], c["pbg"], st, mp, allow)
        fn = g.optimal_interpolation_ensi_multi_ebe if variant == "ebe" else g.optimal_interpolation_ensi_multi_utem
        return fn(b, rs(c["br"]), rs(c["bg"]), rs(c["bgc"]), points, c["pobs"], c["pr"], c["pbg"], c["pbgc"], st, mp, allow)

    def no_observations(which):   # S == 0 inside the library (the Python mirror returns before it): the C entry points themselves
        c, none = ensi_case(1, 9, 8, 5, 1), g.Points(np.zeros(0), np.zeros(0))
        grid, out, barnes = g.Grid(c["lats"], c["lons"]), np.zeros_like(c["bg"]), g.BarnesStructure(20000)
        st = g._structure(barnes)
        if which == "ensi":
            g.check(g.lib().gpp_optimal_interpolation_ensi(grid._h, g._ptr(c["bg"]), 5, none._h, None, None, None, st, 10, 1, g._ptr(out), g._capi.MEM_HOST))
        else:
            g.check(g.lib().gpp_optimal_interpolation_ensi_multi(2, grid._h, None, g._ptr(c["bg"]), None, 5, none._h, None, None, None, None, st, 10, 1,
                                                                 g._ptr(out), g._capi.MEM_HOST))
        assert np.array_equal(out, c["bg"])
        return out

    def oi_huge():   # 700 usable observations at every grid point: the general kernel of optimal_interpolation
        rng = np.random.default_rng(80)
        lats, lons = np.meshgrid(np.linspace(0, 0.1, 4), np.linspace(0, 0.1, 4), indexing="ij")
        plat, plon = 0.1 * rng.random(700), 0.1 * rng.random(700)
        r = lambda *shape: rng.normal(0, 1, shape).astype(F)
        return g.optimal_interpolation(g.Grid(lats, lons), r(4, 4), g.Points(plat, plon), r(700), rng.uniform(0.1, 1, 700).astype(F), r(700), g.BarnesStructure(40000), 0)

    # ---- optimal_interpolation_ensi ----
    base = ensi_case(110, 24, 20, 10, 60)
    report("ensi S == 0", lambda: no_observations("ensi"))
    dead = dict(base, bg=base["bg"].copy()); dead["bg"][3, 4, :] = np.nan
    report("ensi every member invalid", lambda: ensi(dead, 20000, 10))
    one = dict(base, bg=base["bg"].copy()); one["bg"][3, 4, 1:] = np.nan
    report("ensi one valid member (cell count)", lambda: ensi(one, 20000, 10))
    report("ensi scalar structure, Grid, max_points 10", lambda: ensi(base, 20000, 10))
    report("ensi scalar structure, Grid, no extrapolation", lambda: ensi(base, 20000, 10, allow=False))
    report("ensi spatial structure, Grid, max_points 10", lambda: ensi(base, 14000, 10, spatial=True))
    report("ensi Points background", lambda: ensi(base, 20000, 10, points_bg=True))
    report("ensi max_points 0 (big lists)", lambda: ensi(base, 20000, 0))
    report("ensi max_points 40 (big lists)", lambda: ensi(base, 20000, 40))
    twenty = ensi_case(320, 12, 11, 20, 40)
    report("ensi 20 members, k_ensi_members3", lambda: ensi(twenty, 20000, 30))
    with switch("GPP_ENSI_MEMBERS2", "1"):
        report("ensi 20 members, GPP_ENSI_MEMBERS2", lambda: ensi(twenty, 20000, 30))
    report("ensi 80 members", lambda: ensi(ensi_case(380, 12, 11, 80, 40), 20000, 30))
    with switch("GPP_ENSI_PARK_MB", "1"):
        report("ensi GPP_ENSI_PARK_MB=1 (a batch per tile)", lambda: ensi(base, 20000, 10))
    big20, big50 = ensi_case(970, 6, 7, 20, 60), ensi_case(1000, 6, 7, 50, 60)
    report("ensi big-n, 20 members, scalar", lambda: ensi(big20, 200000, 0))
    report("ensi big-n, 50 members, scalar", lambda: ensi(big50, 200000, 0))
    report("ensi big-n, 20 members, spatial", lambda: ensi(big20, 200000, 0, spatial=True))
    report("ensi big-n, 50 members, spatial", lambda: ensi(big50, 200000, 0, spatial=True))
    report("ensi big-n overflow (9000 candidates -> huge list)", lambda: ensi(ensi_case(903, 2, 3, 6, 9000), 300000, 40))
    many = ensi_case(902, 4, 4, 80, 120)
    report("ensi big-n, 80 members (general kernel)", lambda: ensi(many, 200000, 0))
    with switch("GPP_ENSI_NO_BIG", "1"):
        report("ensi GPP_ENSI_NO_BIG with 60 observations", lambda: ensi(big20, 200000, 0))

    # ---- optimal_interpolation_ensi_multi ----
    for v in ("ebe", "ebesc", "utem"):
        c = multi_case(7, v, 300, 12, 70)
        c["bg"][:, 11] = np.nan   # the last member is invalid
        report("multi %s inside the LDS areas, Points" % v, lambda: multi(v, c, 25000, 10, allow=False))
    report("multi ebe inside the LDS areas, Grid", lambda: multi("ebe", multi_case(8, "ebe", 300, 12, 70), 25000, 10, shape=(15, 20)))
    for v, E, S, mp in (("ebe", 10, 140, 100), ("ebesc", 10, 140, 0), ("utem", 9, 700, 0), ("utem", 80, 120, 0)):
        report("multi %s beyond them: %d members, %d obs" % (v, E, S), lambda: multi(v, multi_case(70 + E + S, v, 10, E, S), 200000, mp))
    front = multi_case(9, "ebesc", 300, 10, 70); front["bg"][0, 0] = np.nan
    report("multi ebesc, invalid member in front", lambda: multi("ebesc", front, 25000, 8))
    report("multi S == 0", lambda: no_observations("multi"))

    # ---- the budget of the three general kernels, too small for one workgroup ----
    with switch("GPP_OI_HUGE_BUDGET_MB", "0"):
        report("budget 0: ensi", lambda: ensi(many, 200000, 0))
        report("budget 0: multi ebesc", lambda: multi("ebesc", multi_case(220, "ebesc", 10, 10, 140), 200000, 0))
        report("budget 0: optimal_interpolation", oi_huge)
    report("optimal_interpolation, general kernel", oi_huge)


def parse(d, runlog=None):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    dims = lambda r, k: "x".join(r.get("%s_Size_%s" % (k, a), "?") for a in "XYZ") if ("%s_Size_X" % k) in r else r.get("%s_Size" % k, "?")
    queues = {}
    for r in rows:
        queues.setdefault(r.get("Queue_Id", "0"), []).append("%s grid %s wg %s" % (r["Kernel_Name"], dims(r, "Grid"), dims(r, "Workgroup")))
    print("# %d kernel dispatches on %d queues" % (len(rows), len(queues)))
    for qi, lines in enumerate(queues.values()):   # (queues in the order of their first dispatch)
        print("## queue %d: %d dispatches, sha256 of the ordered list %s" % (qi, len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]))
        i = 0
        while i < len(lines):
            j = i
            while j < len(lines) and lines[j] == lines[i]:
                j += 1
            print("%4d x %s" % (j - i, lines[i]))
            i = j
    if runlog:
        body = open(runlog).read()
        print("## outputs: sha256 of each call's result (or its error), sha256 of these lines %s" % hashlib.sha256(body.encode()).hexdigest()[:16])
        sys.stdout.write(body)


if __name__ == "__main__":
    {"run": run, "parse": lambda: parse(*sys.argv[2:4])}[sys.argv[1]]()
