"""CPU checks that go with tests/test_gpu_oi_union_selection.py:

  * every case of tests/oi_union_selection_cases.py is what it claims, by the oracle: how many cells have more usable observations than
    max_points (and so have to evict), how many have an exact float32 rho tie at the cut and how large the tied group is -- and that the
    oracle's selection takes the LOWER observation indices of such a group;
  * gridpp_amd/csrc/oi_small.h on the host (tools/ubench/oi_small_check.cpp): the triangle-index table of the P build entry by entry
    against the integer definition and the closed form it replaces; d_min_pos / d_min3_pos against fminf, bit for bit, on operands
    without NaN and sign bit (+0, subnormals, +inf among them);
  * a NaN cell or observation coordinate is refused before any kernel runs (so the issue's "NaN cell coordinate" tile cannot be built)."""
import os
import re
import subprocess

import pytest

from tests import oi_union_selection_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_case_is_what_it_claims(name):
    more, tied, biggest, union = K.facts(name)
    print(name, "cells that must choose %d, cells with a tie at the cut %d, largest tied group %d, union of the selections %d" % (more, tied, biggest, union))
    assert (more, tied, biggest) == K.CASES[name][2]
    c = K.build(name)
    assert 1 <= c["plat"].size <= 62


def test_the_cases_cover_the_list():
    mps = {K.mp_of(n) for n in K.CASES}
    assert {1, 2, 8, 9, 31, 32, 40, 50} <= mps                                   # groups that stay empty, K on a group boundary, the wider forms
    unions = {K.facts(n)[3] for n in K.CASES if n.startswith("u")}
    assert unions == {1, 2, 11, 12, 32, 33, 40}                                  # P-build passes: 1 entry .. 13 passes
    assert {K.CASES[n][2][2] for n in K.CASES} >= {0, 2, 3}                       # two and three equal rho at a cut
    first = [n for n in K.CASES if K.mp_of(n) <= 32 and K.facts(n)[3] <= K.DECLINED_UNION and K.CASES[n][2][0] > 0]
    listp = [n for n in K.CASES if K.mp_of(n) <= 32 and K.facts(n)[3] > K.DECLINED_UNION]
    assert len(first) >= 8 and len(listp) >= 4, (first, listp)                   # evictions on the first pass and in the list passes
    assert any(0 < K.CASES[n][2][0] < 64 for n in K.CASES)                        # some cells evict, others only store


def test_small_header_on_the_host(tmp_path):
    exe = str(tmp_path / "oi_small_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "gridpp_amd", "csrc"), os.path.join(ROOT, "tools", "ubench", "oi_small_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    m = re.search(r"table entries (\d+) mismatches (\d+); minima (\d+) mismatches (\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) == 1953 and int(m.group(2)) == 0 and int(m.group(3)) > 5000000 and int(m.group(4)) == 0 and r.returncode == 0, r.stdout


def test_nan_cell_coordinate_never_reaches_a_kernel():
    """A NaN (or infinite) latitude or longitude is refused when the Grid or the Points are made -- `Invalid coords`, as the reference's
    coordinate conversion does (src/api/util.cpp:596-600), for Geodetic and Cartesian sets alike -- so no cell and no observation with a
    NaN coordinate exists for k_oi_union to scan: the no-NaN precondition of d_min_pos cannot be put at risk from that side, and there is
    no such tile to record.  (NaN ELEVATIONS and NaN backgrounds do reach the kernel: the nan_elevation, partial_tile and one_cell cases.)"""
    import numpy as np
    import gridpp_amd as gridpp
    c = K.build("evict_35")
    for bad in (np.nan, np.inf):
        for which in ("lats", "lons"):
            for ctype in (gridpp.Geodetic, gridpp.Cartesian):
                g = {k: np.array(c[k], np.float64) for k in ("lats", "lons")}
                g[which][3, 4] = bad
                with pytest.raises(ValueError, match="Invalid coords"):
                    gridpp.Grid(g["lats"], g["lons"], type=ctype)
                o = {"lats": np.array(c["plat"], np.float64), "lons": np.array(c["plon"], np.float64)}
                o[which][7] = bad
                with pytest.raises(ValueError, match="Invalid coords"):
                    gridpp.Points(o["lats"], o["lons"], type=ctype)
