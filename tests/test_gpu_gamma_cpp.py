"""Builds tests/cpp/test_gamma_api.cpp (a plain g++ program against gridpp_amd/host/gridpp_gamma.hpp + libgridpp_hip.so, the same line as
tests/test_gpu_ldc_cpp.py) and runs it on the GPU box: the reference's known answers and the constructor exceptions through the C++
header, the gamma_inv messages, a Gamma behind a Transform reference and the nested vector forms."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_gamma_header(tmp_path):
    import gridpp_amd   # noqa: F401  (the library is built)
    libdir = os.path.join(ROOT, "gridpp_amd", "lib")
    exe = str(tmp_path / "test_gamma_api")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_gamma_api.cpp"),
           "-L", libdir, "-lgridpp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
