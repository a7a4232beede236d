#!/usr/bin/env python
"""Expected values of the one case of the ensi_multi edge suite whose oracle run is too slow for the suite: utem with 260 members at
2 grid points and 130 observations (tests/ensi_multi_cases.py, "f_utem_260").  The oracle's eigen-solver needs about 11 s for it, the
numpy + LAPACK restatement (tools/make_ensi_multi_fixtures.ensi_multi) 1.5 s; the two agree bit for bit in float32 on this case.

    python tools/make_ensi_multi_edge_fixtures.py   ->  tests/golden/ensi_multi_utem260.npz
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import ensi_multi_cases as K  # noqa: E402


def main():
    c = K.case("f_utem_260")
    expected = K.restatement(c)
    # (the inputs come from the seed; three of them ride along so that the loader notices a builder that no longer produces them)
    np.savez_compressed(K.UTEM260_FIXTURE, expected=expected, background=c["background"], pobs=c["pobs"], plat=c["plat"])
    print("wrote", K.UTEM260_FIXTURE, "%.1f KB" % (os.path.getsize(K.UTEM260_FIXTURE) / 1024))


if __name__ == "__main__":
    sys.exit(main())
