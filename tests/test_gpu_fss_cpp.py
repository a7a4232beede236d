"""Builds tests/cpp/test_fss.cpp (a plain g++ program against gridpp_amd/host/gridpp_fss.hpp + libgridpp_hip.so, the same line as
tests/test_gpu_ranks_cpp.py) and runs it on the GPU box: the two C++ signatures taken by address with their exact types, the default
operator, the hand-worked answers, the shapes that need no device and the exceptions with their messages; then both overloads on a case
written here equal the Python function, bit for bit -- fss too, which both form from the two sums by the one rule (GPP_FSS_VALUE)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, F).ravel().view(np.uint32))


def test_cpp_header_equals_the_python_function(tmp_path):
    import gridpp_amd as gridpp
    libdir = os.path.join(ROOT, "gridpp_amd", "lib")
    exe = str(tmp_path / "test_fss")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_fss.cpp"),
           "-L", libdir, "-lgridpp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    Y, X, E = 37, 70, 6
    rng = np.random.default_rng(422)
    yy, xx = np.meshgrid(np.arange(Y), np.arange(X), indexing="ij")
    smooth = np.sin(yy / 7.0) + np.cos(xx / 11.0)
    cube = (smooth[:, :, None] + rng.normal(0, 0.5, (Y, X, E))).astype(F)
    ref = (smooth + rng.normal(0, 0.5, (Y, X))).astype(F)
    cube[rng.random(cube.shape) < 0.08] = np.nan
    cube[5, 7], cube[20, 30, 1:] = np.inf, -np.inf        # a cell without a valid member, a cell with one
    ref[rng.random(ref.shape) < 0.04] = np.inf
    case = tmp_path / "case.txt"
    case.write_text("\n".join(["%d %d %d" % (Y, X, E)] + [bits(a) for a in (cube, ref)]) + "\n")
    out = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0].split("_")[0] in ("field", "cube"):
            got[w[0]] = np.array([int(v, 16) for v in w[2:]], np.uint64)
            assert got[w[0]].size == int(w[1])
    thr, hws = [-0.2, 0.4, 1.0], [0, 2, 16, 40]
    want = {"field_gt": gridpp.fractions_skill_score(cube[:, :, 0], ref, thr, hws), "field_lt": gridpp.fractions_skill_score(cube[:, :, 0], ref, thr, hws, gridpp.Lt),
            "cube_gt": gridpp.fractions_skill_score(cube, ref, thr, hws, gridpp.Gt), "cube_geq": gridpp.fractions_skill_score(cube, ref, thr, hws, gridpp.Geq)}
    assert set(got) == {"%s_%s" % (k, p) for k in want for p in ("fss", "fbs", "worst", "cells")}
    for name, res in want.items():
        assert res.cells.all() and not np.isnan(res.fss).any(), name
        for part, a in (("fss", res.fss), ("fbs", res.fbs), ("worst", res.fbs_worst), ("cells", res.cells)):
            np.testing.assert_array_equal(got["%s_%s" % (name, part)], np.ascontiguousarray(a).ravel().view(np.uint64), err_msg=name + " " + part)
