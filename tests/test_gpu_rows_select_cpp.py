"""Builds tests/cpp/test_rows_select_api.cpp (a plain g++ program against gridpp_amd/host/gridpp.hpp + libgridpp_hip.so, the same line as
tests/test_gpu_window_cpp.py) and runs it on the GPU box: calc_statistic(vec2), calc_quantile(vec2, q) and calc_quantile(vec3, vec2)
through the C++ drop-in boundary, with ragged and empty rows, the default quantile and the exceptions."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_rows_select_overloads(tmp_path):
    libdir = os.path.join(ROOT, "gridpp_amd", "lib")
    exe = str(tmp_path / "test_rows_select_api")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_rows_select_api.cpp"),
           "-L", libdir, "-lgridpp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
