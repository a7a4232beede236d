"""Builds tests/cpp/test_members.cpp (a plain g++ program against gridpp_amd/host/gridpp_members.hpp + libgridpp_hip.so, the same line as
tests/test_gpu_nbh_quantiles_cpp.py) and runs it on the GPU box: the signatures taken by address with their exact types, known answers, the
empty shapes and the exceptions with their messages, every plane against neighbourhood / calc_gradient of gridpp.hpp; then the vec3 overloads
and the device-pointer forms of neighbourhood_members and calc_gradient_members on one exact-data cube equal the Python functions, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import members_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
STATS = ["Mean", "Sum", "Count", "Min", "Max", "Std", "Variance"]


def bits(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, F).ravel().view(np.uint32))


def test_cpp_header_equals_the_python_functions(tmp_path):
    import gridpp_amd as gridpp
    libdir = os.path.join(ROOT, "gridpp_amd", "lib")
    exe = str(tmp_path / "test_members")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_members.cpp"),
           "-L", libdir, "-lgridpp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    shape, hw = (21, 37, 8), 3
    cube, per = R.exact_cube(41, shape), R.exact_cube(42, shape)
    rng = np.random.default_rng(43)
    shared = (rng.integers(-512, 513, shape[:2]) / 8).astype(F)
    shared[rng.random(shape[:2]) < 0.05] = np.nan
    case = tmp_path / "case.txt"
    case.write_text("\n".join(["%d %d %d %d" % (shape + (hw,))] + [bits(a) for a in (cube, shared, per)]) + "\n")
    out = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "all checks passed" in out.stdout
    want = {}
    for name in STATS:
        want[name] = want[name + "_device"] = gridpp.neighbourhood_members(cube, hw, getattr(gridpp, name))
    for name in ("MinMax", "LinearRegression"):
        gt = getattr(gridpp, name)
        want[name + "_shared"] = want[name + "_shared_device"] = gridpp.calc_gradient_members(shared, cube, gt, hw, 2, np.nan, 0)
        want[name + "_per"] = want[name + "_per_device"] = gridpp.calc_gradient_members(per, cube, gt, hw, 3, 1.0, -0.5)
    got = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0] in want:
            got[w[0]] = np.array([int(v, 16) for v in w[2:]], np.uint32)
            assert got[w[0]].size == int(w[1])
    assert set(got) == set(want)
    assert np.isnan(want["Mean"]).any() and not np.isnan(want["Mean"]).all() and (want["LinearRegression_per"] != F(-0.5)).any()
    for name, a in want.items():
        w = np.ascontiguousarray(a, F).ravel()
        g = got[name].view(F)
        assert g.shape == w.shape, name
        assert (np.isnan(g) == np.isnan(w)).all(), name
        np.testing.assert_array_equal(got[name][~np.isnan(w)], w.view(np.uint32)[~np.isnan(w)], err_msg=name)
