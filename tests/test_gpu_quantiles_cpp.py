"""Builds tests/cpp/test_quantiles.cpp (a plain g++ program against gridpp_amd/host/gridpp_quantiles.hpp + libgridpp_hip.so, the same line
as tests/test_gpu_oi_gain_cpp.py) and runs it on the GPU box: the four C++ signatures taken by address with their exact types, known
answers, a ragged vec2, the empty shapes and the exceptions with their messages; then the vector, rows, cube and ragged forms of
calc_quantiles and both curves of quantile_mapping_curves on a case written here equal the Python functions, bit for bit."""
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
    exe = str(tmp_path / "test_quantiles")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_quantiles.cpp"),
           "-L", libdir, "-lgridpp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    Y, X, Tr, Tf = 3, 5, 40, 33
    rng = np.random.default_rng(21)
    ref, fcst = rng.normal(5, 2, (Y, X, Tr)).astype(F), rng.gamma(2, 2, (Y, X, Tf)).astype(F)
    ref[rng.random(ref.shape) < 0.05] = np.nan
    fcst[rng.random(fcst.shape) < 0.05] = np.inf
    ref[2, 1], fcst[2, 1, 1:] = np.nan, np.nan        # a cell of all-NaN, a cell with one valid value
    ref[0, 0, :4] = [0.0, -0.0, -50.0, 50.0]
    levels = np.array([0.5, 0.0, 0.1, 1.0, np.nan, 0.9, 0.5, 0.25], F)
    knots = np.linspace(0, 1, 8, dtype=F)             # quantile_mapping_curves takes no NaN level: the curves get levels of their own
    case = tmp_path / "case.txt"
    case.write_text("\n".join(["%d %d %d %d %d %d" % (Y, X, Tr, Tf, levels.size, knots.size)] + [bits(a) for a in (ref, fcst, levels, knots)]) + "\n")
    out = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0] in ("vec", "rows", "cube", "ragged", "curve_ref", "curve_fcst"):
            got[w[0]] = np.array([int(v, 16) for v in w[2:]], np.uint32)
            assert got[w[0]].size == int(w[1])
    ragged = ref[1].copy()
    for x in range(X):
        ragged[x, Tr - x:] = np.nan                   # the C++ side pads the shorter rows with NaN
    curve_ref, curve_fcst = gridpp.quantile_mapping_curves(ref, fcst, knots)
    want = {"vec": gridpp.calc_quantiles(ref[0, 0], levels), "rows": gridpp.calc_quantiles(ref[0], levels), "cube": gridpp.calc_quantiles(ref, levels),
            "ragged": gridpp.calc_quantiles(ragged, levels), "curve_ref": curve_ref, "curve_fcst": curve_fcst}
    assert set(got) == set(want)
    for name, a in want.items():
        w = np.ascontiguousarray(a, F).ravel()
        g = got[name].view(F)
        assert g.shape == w.shape, name
        assert (np.isnan(g) == np.isnan(w)).all(), name
        np.testing.assert_array_equal(got[name][~np.isnan(w)], w.view(np.uint32)[~np.isnan(w)], err_msg=name)
