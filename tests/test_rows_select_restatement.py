"""tests/rows_select_ref.py (the numpy restatement the GPU selection paths are held to) against the CPU oracle's calc_quantile, bit for
bit.  The one exemption: where both values are zero their signs may differ -- the reference sorts with std::sort, under which -0.0 and
+0.0 are equivalent and their order is unspecified, while the restatement (and the GPU) ranks -0.0 below +0.0.  The exemption must stay
rare: it is used in fewer than 1 % of the comparisons."""
import numpy as np

from tests import rows_select_ref as ref
from tests.test_gpu_neighbourhood_edges import QUANTILES, rows

LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 159, 160, 161, 255, 256, 257, 1000, 4097]
LEVELS = QUANTILES + [0.25, 0.9]


def test_restatement_equals_the_oracle():
    from oracle import oracle as O
    compared = exempt = 0
    for L in LENGTHS:
        a = np.concatenate([rows(L), ref.adversarial(L)])
        for q in LEVELS:
            for r in a:
                got, want = np.float32(ref.quantile(r, q)), np.float32(O.calc_quantile(r, q))
                compared += 1
                if np.isnan(want):
                    assert np.isnan(got), (L, q)
                    continue
                if got.view(np.uint32) != want.view(np.uint32):
                    assert got == 0 and want == 0, (L, q, got, want)
                    exempt += 1
    print("comparisons: %d, sign-of-zero exemptions: %d" % (compared, exempt))
    assert compared == len(LENGTHS) * len(LEVELS) * 79
    assert exempt < 0.01 * compared
