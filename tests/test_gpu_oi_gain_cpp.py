"""Builds tests/cpp/test_oi_gain.cpp (a plain g++ program against gridpp_amd/host/gridpp_oi_gain.hpp + libgridpp_hip.so, the same line as
tests/test_gpu_ldc_cpp.py) and runs it on the GPU box: gridpp::OiGain for a Grid and for a Points background, one field and a stack of
17, clamped and not, and the analysis variance; every result equals the Python binding's, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_oi_parity import make_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, F).ravel().view(np.uint32))


def test_cpp_class_equals_the_python_binding(tmp_path):
    import gridpp_amd as gridpp
    libdir = os.path.join(ROOT, "gridpp_amd", "lib")
    exe = str(tmp_path / "test_oi_gain")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_oi_gain.cpp"),
           "-L", libdir, "-lgridpp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    Y, X, S, E = 21, 27, 90, 17
    c = make_case(5, Y, X, S)
    lats, lons, plat, plon = (a.astype(F) for a in (c["lats"], c["lons"], c["plat"], c["plon"]))
    rng = np.random.default_rng(8)
    stack = rng.normal(0, 1, (Y, X, E)).astype(F)
    pbg = rng.normal(0, 1, (S, E)).astype(F)
    case = tmp_path / "case.txt"
    case.write_text("\n".join(["%d %d %d %d" % (Y, X, S, E)] + [bits(a) for a in (lats, lons, plat, plon, c["ratios"], stack, c["obs"], pbg)]) + "\n")
    out = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and (w[0].startswith("grid_") or w[0].startswith("points_")):
            got[w[0]] = np.array([int(v, 16) for v in w[2:]], np.uint32)
            assert got[w[0]].size == int(w[1])
    st = gridpp.BarnesStructure(12000)
    points = gridpp.Points(plat, plon)
    gain = gridpp.optimal_interpolation_gain(gridpp.Grid(lats, lons), points, c["ratios"], st, 12)
    pgain = gridpp.optimal_interpolation_gain(gridpp.Points(lats.ravel(), lons.ravel()), points, c["ratios"], st, 12)
    want = {"grid_one": gain.apply(stack[..., 0], c["obs"], pbg[:, 0]), "grid_stack": gain.apply(stack, c["obs"], pbg),
            "grid_clamped": gain.apply(stack, c["obs"], pbg, False), "grid_variance": gain.analysis_variance(np.full((Y, X), 1.5, F)),
            "points_one": pgain.apply(stack[..., 0].ravel(), c["obs"], pbg[:, 0]), "points_stack": pgain.apply(stack.reshape(Y * X, E), c["obs"], pbg),
            "points_variance": pgain.analysis_variance(np.full(Y * X, 1.5, F))}
    assert set(got) == set(want)
    for name, a in want.items():
        np.testing.assert_array_equal(got[name], np.ascontiguousarray(a).ravel().view(np.uint32), err_msg=name)
    assert (got["grid_clamped"] != got["grid_stack"]).any()
    # a Grid and the same points as a Points set tile differently (8 x 8 blocks / runs of 64): the analyses agree to the measure of the suite
    a, b = want["grid_stack"].ravel().astype(np.float64), want["points_stack"].ravel().astype(np.float64)
    assert np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3)) < 1e-5
