"""Records tests/golden/oi_union_split_rows_parent.npz: analyses and variances (float32) of the tiles of tests/oi_union_split_cases.py as the
library computes them WITHOUT the split rows -- run it on the GPU against a build of the commit before the split, or one with
-DGPP_UNION_SPLIT=0:

    GPP_LIB=/path/to/that/libgridpp_hip.so python tools/make_oi_union_split_rows_golden.py [OUT.npz]

Every first-pass case asserts oi_last_stats()["fallback_tiles"] == 0 while it is recorded (tests/oi_union_split_cases.py:record), so that a
declined tile cannot make the comparison of tests/test_gpu_oi_union_split_rows.py vacuous."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tests import oi_union_split_cases as K


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "oi_union_split_rows_parent.npz")
    rec = K.record()
    assert all(v.dtype == np.float32 for v in rec.values())
    np.savez_compressed(out, **rec)
    print("%d arrays, %d values, %d bytes -> %s" % (len(rec), sum(v.size for v in rec.values()), os.path.getsize(out), out))


if __name__ == "__main__":
    main()
