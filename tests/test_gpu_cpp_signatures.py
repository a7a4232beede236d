"""Builds tests/cpp/test_signatures.cpp (plain g++ against gridpp_amd/host/gridpp.hpp + libgridpp_hip.so) and runs it once on the
GPU: the class surface of include/gridpp.h -- Point, KDTree, Points, Grid, the structure functions with their spatially varying
constructors -- with the reference's known answers, corr against a vector bit-equal to the scalar calls, a clone that outlives
its original, and an optimal_interpolation with a spatially varying BarnesStructure (the k_oi_union_sp family, which a C++ host
could not reach before) against the values the python mirror returns for the same inputs, handed over in a file."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _analysis_file(path):
    import gridpp_amd as gridpp
    rng = np.random.default_rng(77)
    Y = X = 40
    S = 60
    lats, lons = np.meshgrid(np.linspace(59.5, 60.5, Y), np.linspace(9.0, 11.0, X), indexing="ij")
    lats, lons = lats.astype(np.float32), lons.astype(np.float32)
    h = (20000 * (1 + 0.3 * np.sin(np.arange(Y * X) * 0.37))).reshape(Y, X).astype(np.float32)
    background = rng.normal(0, 1, (Y, X)).astype(np.float32)
    plats, plons = rng.uniform(59.5, 60.5, S).astype(np.float32), rng.uniform(9.0, 11.0, S).astype(np.float32)
    pobs, pratios = rng.normal(0, 1, S).astype(np.float32), rng.uniform(0.1, 1, S).astype(np.float32)
    grid, points = gridpp.Grid(lats, lons), gridpp.Points(plats, plons)
    pbackground = gridpp.nearest(grid, points, background)
    zeros = np.zeros((Y, X), np.float32)
    expected = gridpp.optimal_interpolation(grid, background, points, pobs, pratios, pbackground, gridpp.BarnesStructure(grid, h, zeros, zeros), 20)
    assert np.isfinite(expected).all() and np.count_nonzero(expected != background) > 400
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (Y, X, S))
        for a in (lats, lons, h, background, expected, plats, plons, pobs, pratios, pbackground):
            f.write(" ".join("%.9g" % v for v in np.asarray(a, np.float32).ravel()) + "\n")   # (9 digits: a float32 reads back exactly)


def test_cpp_class_surface(tmp_path):
    libdir = os.path.join(ROOT, "gridpp_amd", "lib")
    exe = str(tmp_path / "test_signatures")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_signatures.cpp"),
           "-L", libdir, "-lgridpp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    analysis = str(tmp_path / "analysis.txt")
    _analysis_file(analysis)
    out = subprocess.run([exe, analysis], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
