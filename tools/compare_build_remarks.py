"""Per-kernel resource usage of two builds, side by side: the build/obj/*.o.remarks files that build() keeps (-Rpass-analysis=kernel-resource-usage)
of a checkout of the parent commit and of this tree.

    python tools/compare_build_remarks.py PARENT_TREE [THIS_TREE] > profiles/<name>_build_remarks.txt

One line per unit and kernel: VGPRs, AGPRs, SGPRs, scratch, LDS and occupancy of both, `equal` or `DIFFERS`; a kernel only one build has is `removed` /
`added`.  Instances of rocprim / hipcub templates are counted per unit and compared as sorted lists, not listed.  Exit status 1 when anything differs.
"""
import glob
import os
import subprocess
import sys

FIELDS = (("VGPRs:", "VGPRs"), ("AGPRs:", "AGPRs"), ("TotalSGPRs:", "SGPRs"), ("ScratchSize [bytes/lane]:", "scratch"), ("LDS Size [bytes/block]:", "LDS"),
          ("Occupancy [waves/SIMD]:", "occupancy"))


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt", "-p"] + names, capture_output=True, text=True)
    short = out.stdout.splitlines() if out.returncode == 0 else names
    return dict(zip(names, short))


def kernels(path):
    """{mangled name: tuple of the six figures} of one remarks file"""
    res, name, cur = {}, None, {}
    with open(path) as f:
        for l in f:
            if "Function Name:" in l:
                name = l.split("Function Name:")[1].split()[0]
                cur = res.setdefault(name, {})
            elif name:
                for key, _ in FIELDS:
                    if key in l:
                        cur[key] = int(l.split(key)[1].split()[0])
    return {k: tuple(v.get(key, -1) for key, _ in FIELDS) for k, v in res.items()}


def main():
    parent = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    units = sorted({os.path.basename(p)[:-len(".o.remarks")] for t in (parent, this) for p in glob.glob(os.path.join(t, "build", "obj", "*.o.remarks"))})
    lines, differ, total = [], 0, 0
    for u in units:
        a = kernels(os.path.join(parent, "build", "obj", u + ".o.remarks")) if os.path.exists(os.path.join(parent, "build", "obj", u + ".o.remarks")) else {}
        b = kernels(os.path.join(this, "build", "obj", u + ".o.remarks")) if os.path.exists(os.path.join(this, "build", "obj", u + ".o.remarks")) else {}
        names = demangle(sorted(set(a) | set(b)))
        lib = lambda n: "rocprim" in n or "hipcub" in n
        own = sorted((n for n in names if not lib(n)), key=lambda n: names[n])
        for n in own:
            total += 1
            show = names[n].replace("(anonymous namespace)::", "").replace("gpp::", "")
            fmt = lambda t: " ".join("%5d" % v for v in t)
            if n not in b:
                lines.append("%-20s %-72s removed (parent: %s)" % (u, show, fmt(a[n]))); differ += 1
            elif n not in a:
                lines.append("%-20s %-72s added (this tree: %s)" % (u, show, fmt(b[n]))); differ += 1
            else:
                same = a[n] == b[n]
                differ += not same
                lines.append("%-20s %-72s %s | %s  %s" % (u, show, fmt(a[n]), fmt(b[n]), "equal" if same else "DIFFERS"))
        la, lb = sorted((n, a[n]) for n in a if lib(n)), sorted((n, b[n]) for n in b if lib(n))
        if la or lb:
            same = la == lb
            differ += not same
            lines.append("%-20s %-72s %d | %d  %s" % (u, "(rocprim / hipcub instances: names and figures)", len(la), len(lb), "equal" if same else "DIFFERS"))
    print("# %d units, %d kernels of the library's own, %d lines that differ" % (len(units), total, differ))
    print("# unit, kernel, parent: %s | this tree: the same six" % " ".join(s for _, s in FIELDS))
    print("\n".join(lines))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
