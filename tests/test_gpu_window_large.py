"""GPU: gridpp.window on a matrix of more than 2^31 values, the one size at which a 32-bit offset shows.  Apart from the rest of the
parity tests because of what it needs: 8.6 GB for the matrix, as much for a result, and on the general path of the scan statistics two
planes of that size from the workspace pool -- 34 GB of HBM at the peak, a second or two of kernels."""
import contextlib

import pytest

from tests import window_ref as R

pytestmark = pytest.mark.gpu

from gridpp_amd import _capi   # noqa: E402

ROWS = _capi.WINDOW_TILE_ROWS


@pytest.fixture(scope="module")
def gridpp():
    import gridpp_amd
    if gridpp_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return gridpp_amd


@contextlib.contextmanager
def general_path():
    lib = _capi.lib()
    assert lib.gpp_set_path_override(b"GPP_WINDOW_GENERAL", b"1") == _capi.GPP_OK
    try:
        yield
    finally:
        lib.gpp_set_path_override(b"GPP_WINDOW_GENERAL", None)


def test_offsets_beyond_two_to_the_31(gridpp):
    """Y * T just above 2^31 values: the last rows are only right with 64-bit offsets, and the flat grids of the general path reach
    them through their grid-stride loop.  Rows are independent, so the restatement of the first and the last rows is the whole check.
    One result is alive at a time."""
    import torch
    T = 64
    Y = (1 << 31) // T + ROWS + 1
    free, _ = torch.cuda.mem_get_info()
    assert free > 4.5 * Y * T * 4, "this test needs 34 GB of free HBM"
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    d = torch.rand((Y, T), device="cuda", generator=gen)
    d[-5, 3] = float("nan")
    head, tail = d[:2].cpu().numpy(), d[-(ROWS + 3):].cpu().numpy()

    def check(statistic, length, before):
        out = gridpp.window(d, length, statistic, before)
        assert out.shape == d.shape
        first, last = out[:2].cpu().numpy(), out[-(ROWS + 3):].cpu().numpy()
        del out
        R.same_bits(first, R.window(head, length, statistic, before))
        R.same_bits(last, R.window(tail, length, statistic, before))

    try:
        check(R.Sum, 24, True)
        check(R.Max, 7, False)
        with general_path():
            check(R.Sum, 24, True)
            check(R.Max, 7, False)
    finally:
        del d
        torch.cuda.empty_cache()
        gridpp._capi.lib().gpp_release_workspaces()
