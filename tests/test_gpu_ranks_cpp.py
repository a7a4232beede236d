"""Builds tests/cpp/test_ranks.cpp (a plain g++ program against gridpp_amd/host/gridpp_ranks.hpp + libgridpp_hip.so, the same line as
tests/test_gpu_quantiles_cpp.py) and runs it on the GPU box: the twelve C++ signatures taken by address with their exact types, known
answers, a ragged vec2, the empty shapes and the exceptions with their messages; then the vector, rows, cube and ragged forms of the four
functions on a case written here equal the Python functions, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, F).ravel().view(np.uint32))


def test_cpp_header_equals_the_python_functions(tmp_path):
    import gridpp_amd as gridpp
    libdir = os.path.join(ROOT, "gridpp_amd", "lib")
    exe = str(tmp_path / "test_ranks")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_ranks.cpp"),
           "-L", libdir, "-lgridpp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    Y, X, E = 3, 5, 40
    rng = np.random.default_rng(22)
    vals, tmpl = rng.gamma(0.7, 2, (Y, X, E)).astype(F), rng.normal(5, 2, (Y, X, E)).astype(F)
    vals[vals < 0.3] = 0.0                               # tied zeros ...
    vals[(vals == 0) & (rng.random(vals.shape) < 0.5)] = -0.0   # ... of either sign
    vals[rng.random(vals.shape) < 0.05] = np.nan
    tmpl[rng.random(tmpl.shape) < 0.05] = np.inf
    vals[2, 1], tmpl[2, 2, 1:] = np.nan, np.nan          # a cell of all-NaN, a template cell with one valid value
    ref = rng.gamma(0.7, 2, (Y, X)).astype(F)
    ref[0, 1], ref[0, 2] = np.nan, np.inf
    case = tmp_path / "case.txt"
    case.write_text("\n".join(["%d %d %d" % (Y, X, E)] + [bits(a) for a in (vals, tmpl, ref)]) + "\n")
    out = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0].split("_")[0] in ("ranks", "sorted", "reorder", "crps"):
            got[w[0]] = np.array([int(v, 16) for v in w[2:]], np.uint32)
            assert got[w[0]].size == int(w[1])
    ragged = vals[1].copy()
    for x in range(X):
        ragged[x, E - x:] = np.nan                       # the C++ side pads the shorter rows with NaN and cuts the results back
    cut = lambda a: np.concatenate([a[x, :E - x] for x in range(X)])
    want = {"ranks_vec": gridpp.calc_ranks(vals[0, 0]), "ranks_rows": gridpp.calc_ranks(vals[0]), "ranks_cube": gridpp.calc_ranks(vals),
            "sorted_vec": gridpp.sort_rows(vals[0, 0]), "sorted_rows": gridpp.sort_rows(vals[0]), "sorted_cube": gridpp.sort_rows(vals),
            "reorder_vec": gridpp.reorder_by_ranks(vals[0, 0], tmpl[0, 0]), "reorder_rows": gridpp.reorder_by_ranks(vals[0], tmpl[0]),
            "reorder_cube": gridpp.reorder_by_ranks(vals, tmpl),
            "crps_vec": gridpp.calc_crps(vals[0, 0], ref[0, 0]), "crps_rows": gridpp.calc_crps(vals[0], ref[0]), "crps_cube": gridpp.calc_crps(vals, ref),
            "ranks_ragged": cut(gridpp.calc_ranks(ragged)), "sorted_ragged": cut(gridpp.sort_rows(ragged)), "crps_ragged": gridpp.calc_crps(ragged, ref[1])}
    assert set(got) == set(want)
    for name, a in want.items():
        if name.startswith("ranks"):
            np.testing.assert_array_equal(got[name].view(np.int32), np.asarray(a, np.int32).ravel(), err_msg=name)
            continue
        w = np.ascontiguousarray(a, F).ravel()
        g = got[name].view(F)
        assert g.shape == w.shape, name
        assert (np.isnan(g) == np.isnan(w)).all(), name
        np.testing.assert_array_equal(got[name][~np.isnan(w)], w.view(np.uint32)[~np.isnan(w)], err_msg=name)
