"""Builds tests/cpp/test_downscale_plan_cube.cpp (a plain g++ program against gridpp_amd/host/gridpp_downscale_plan.hpp +
libgridpp_hip.so, the same line as tests/test_gpu_downscale_plan_cpp.py) and runs it on the GPU box: the cube-layout gradients of
gridpp::DownscalingPlan for a Grid and for a Points output and its ensemble downscalers, each equal to the direct function of
gridpp.hpp bit for bit."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_cube_methods_equal_the_direct_calls(tmp_path):
    import gridpp_amd  # noqa: F401  (the library is built)
    libdir = os.path.join(ROOT, "gridpp_amd", "lib")
    exe = str(tmp_path / "test_downscale_plan_cube")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_downscale_plan_cube.cpp"),
           "-L", libdir, "-lgridpp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
