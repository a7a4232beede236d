"""Records tests/golden/oi_union_selection_parent.npz: the analyses (float32) of the cases of tests/oi_union_selection_cases.py as the
library of the commit BEFORE the round-12 changes of k_oi_union computes them (no minima without NaN handling, no triangle-index table) --
run it on the GPU against a build of that commit:

    GPP_LIB=/path/to/that/libgridpp_hip.so python tools/make_oi_union_selection_golden.py [OUT.npz]

Every case also runs under GPP_OI_NO_BULK_CERT while it is recorded and must give the same bits there (tests/oi_union_selection_cases.py:record)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tests import oi_union_selection_cases as K


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "oi_union_selection_parent.npz")
    rec = K.record()
    assert all(v.dtype == np.float32 for v in rec.values())
    np.savez_compressed(out, **rec)
    print("%d arrays, %d values, %d bytes -> %s" % (len(rec), sum(v.size for v in rec.values()), os.path.getsize(out), out))


if __name__ == "__main__":
    main()
