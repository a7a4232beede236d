"""CPU-only: tests/cpp/test_signatures.cpp pins the exact type of every member and function of the class surface of
include/gridpp.h (Point, KDTree, Points, Grid, the structure functions and their spatially varying constructors, the container
helpers) on gridpp_amd/host/gridpp.hpp.  Checking the syntax needs the two headers only: no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signatures_compile():
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(ROOT, "gridpp_amd", "host"),
           os.path.join(ROOT, "tests", "cpp", "test_signatures.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
