"""Builds tests/cpp/test_metric_optimizer_api.cpp (a plain g++ program against gridpp_amd/host/gridpp_metric_optimizer.hpp +
libgridpp_hip.so, the same line as tests/test_gpu_gamma_cpp.py) and runs it on the GPU box: the reference's two known answers, the exact
values of DESIGN.md 4.13 for them, dropped thresholds, the cases without device work and both exceptions through the C++ header."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_metric_optimizer_header(tmp_path):
    import gridpp_amd   # noqa: F401  (the library is built)
    libdir = os.path.join(ROOT, "gridpp_amd", "lib")
    exe = str(tmp_path / "test_metric_optimizer_api")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_metric_optimizer_api.cpp"),
           "-L", libdir, "-lgridpp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
