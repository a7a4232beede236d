"""Builds tests/cpp/test_nbh_quantiles.cpp (a plain g++ program against gridpp_amd/host/gridpp_nbh_quantiles.hpp + libgridpp_hip.so, the same
line as tests/test_gpu_quantiles_cpp.py) and runs it on the GPU box: the signatures taken by address with their exact types, known answers,
the empty shapes and the exceptions with their messages, every level plane against neighbourhood_quantile_fast of gridpp.hpp; then the 3-D,
2-D and device-pointer forms of neighbourhood_quantiles_fast and neighbourhood_cdf on a case written here equal the Python functions, bit
for bit."""
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
    exe = str(tmp_path / "test_nbh_quantiles")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_nbh_quantiles.cpp"),
           "-L", libdir, "-lgridpp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    Y, X, E, hw = 21, 37, 8, 3
    rng = np.random.default_rng(23)
    cube = rng.uniform(0, 10, (Y, X, E)).astype(F)
    cube[rng.random(cube.shape) < 0.05] = np.nan
    cube[rng.random(cube.shape) < 0.02] = np.inf
    cube[8:16, 10:20, :] = np.nan                     # windows without a valid cell
    levels = np.array([0.5, 0.0, 0.1, 1.0, np.nan, 0.9, 0.5, 0.25], F)
    thr = np.array([0.0, 2.5, 1.0, 5.0, 5.0, 7.5, 10.0], F)     # unsorted, with a duplicate
    case = tmp_path / "case.txt"
    case.write_text("\n".join(["%d %d %d %d %d %d" % (Y, X, E, levels.size, thr.size, hw)] + [bits(a) for a in (cube, levels, thr)]) + "\n")
    out = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "all checks passed" in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0] in ("levels3", "cdf3", "levels2", "cdf2", "levels3_device", "cdf3_device"):
            got[w[0]] = np.array([int(v, 16) for v in w[2:]], np.uint32)
            assert got[w[0]].size == int(w[1])
    plane = np.ascontiguousarray(cube[:, :, 0])
    lv3, cdf3 = gridpp.neighbourhood_quantiles_fast(cube, levels, hw, thr), gridpp.neighbourhood_cdf(cube, thr, hw)
    want = {"levels3": lv3, "cdf3": cdf3, "levels2": gridpp.neighbourhood_quantiles_fast(plane, levels, hw, thr), "cdf2": gridpp.neighbourhood_cdf(plane, thr, hw),
            "levels3_device": lv3, "cdf3_device": cdf3}
    assert set(got) == set(want)
    assert np.isnan(lv3).any() and not np.isnan(lv3[:, :, 0]).all()
    for name, a in want.items():
        w = np.ascontiguousarray(a, F).ravel()
        g = got[name].view(F)
        assert g.shape == w.shape, name
        assert (np.isnan(g) == np.isnan(w)).all(), name
        np.testing.assert_array_equal(got[name][~np.isnan(w)], w.view(np.uint32)[~np.isnan(w)], err_msg=name)
