"""Builds tests/cpp/test_ldc_api.cpp (a plain g++ program against gridpp_amd/host/gridpp.hpp + libgridpp_hip.so, the same line as
tests/test_gpu_window_cpp.py) and runs it on the GPU box: both local_distribution_correction overloads of the C++ drop-in boundary
on fixture A of tests/ldc_ref.py, handed over as text; their output equals the Python binding's, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import ldc_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, F).ravel().view(np.uint32))


def test_cpp_overloads_equal_the_python_binding(tmp_path):
    import gridpp_amd as gridpp
    libdir = os.path.join(ROOT, "gridpp_amd", "lib")
    exe = str(tmp_path / "test_ldc_api")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_ldc_api.cpp"),
           "-L", libdir, "-lgridpp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    fx = R.FixtureA(rounded=True)
    Y, X = fx.lats.shape
    T, S = fx.pobs.shape
    case = tmp_path / "fixture_a.txt"
    case.write_text("\n".join(["%d %d %d %d" % (Y, X, S, T)] + [bits(a) for a in (fx.lats, fx.lons, fx.bg, fx.py, fx.px, fx.pobs, fx.pbg)]) + "\n")
    out = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0] in ("times", "single"):
            got[w[0]] = np.array([int(v, 16) for v in w[3:]], np.uint32).reshape(int(w[1]), int(w[2]))
    grid, points = fx.device_points(gridpp)
    st = gridpp.BarnesStructure(2500)
    times = gridpp.local_distribution_correction(grid, fx.bg, points, fx.pobs, fx.pbg, st, 0.1, 0.9, 5)
    single = gridpp.local_distribution_correction(grid, fx.bg, points, fx.pobs[0], fx.pbg[0], st, 0.1, 0.9, 5)
    np.testing.assert_array_equal(got["times"], times.view(np.uint32))
    np.testing.assert_array_equal(got["single"], single.view(np.uint32))
    assert (times.view(np.uint32) != single.view(np.uint32)).any()
