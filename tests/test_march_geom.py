"""Builds tests/cpp/test_march_geom.cpp with g++ alone (gridpp_amd/csrc/march_geom.h includes only the standard library) and runs it: the shared
segment geometry of the marching kernels gives the segment height and count of the three formulas it replaced (MarchGeom of neighbourhood.hip,
gpp_neighbourhood_score, FssCall::march) for Y = 1 .. 300, 4000 and the three heights around 65535 chunks, 1 .. 70 strips, 1 / 3 / 100 planes and
fill targets 1, 3, 768, 1024, 1280 at the chunk height 32: no launch of those kernels changed its grid.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_march_segments_match_the_three_parent_formulas(tmp_path):
    exe = str(tmp_path / "test_march_geom")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "gridpp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_march_geom.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
    assert "%d cases" % (304 * 70 * 5 * 5) in out.stdout   # the whole sweep ran
