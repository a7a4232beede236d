"""GPU: gridpp.window against the float32 restatement of tests/window_ref.py, which tests/test_window_restatement.py pins to the
reference's own known answers.

Bit for bit (NaNs in the same places), no tolerance: both sides perform the same float32 operations in the same order -- the kernels
add along a row sequentially like the reference (src/api/window.cpp:33-111), the library is built with -ffp-contract=off and
correctly rounded division and square root.  RandomChoice has no one answer: every output must be a valid member of its window.

R x C is the tile of the fused kernels (GPP_WINDOW_TILE_ROWS x GPP_WINDOW_TILE_COLS), SPAN the largest back + lead a fused call may
have (GPP_WINDOW_FUSED_SPAN): the shapes and lengths below sit on both sides of each.  Every case runs from numpy arrays (the host
path) on the path the library picks, and again from torch tensors (the device path) under GPP_WINDOW_GENERAL, the override that forces
the general path."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import window_ref as R

pytestmark = pytest.mark.gpu

from gridpp_amd import _capi   # noqa: E402

ROWS, COLS, SPAN = _capi.WINDOW_TILE_ROWS, _capi.WINDOW_TILE_COLS, _capi.WINDOW_FUSED_SPAN
EXACT = (R.Mean, R.Sum, R.Count, R.Min, R.Max, R.Median, R.Std, R.Variance)
ARRAY_CASES = [c for c in R.CASES if R.needs_device(c)]
YS = (1, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 3)
TS = (1, 2, COLS - 1, COLS, COLS + 1, 2 * COLS + 3)
CONTENTS = ("full", "sprinkled", "nan_at_0", "all_nan_row", "mixed_magnitude")
FLAGS = ((False, False), (False, True), (True, False), (True, True))   # keep_missing, missing_edges
FUSED_CENTRED, FUSED_BEFORE = SPAN, SPAN + 1   # the largest fused lengths: h + roundup4(h) <= SPAN with h = 15; length - 1 <= SPAN


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
        buf = C.create_string_buffer(256)
        assert lib.gpp_active_overrides(buf, 256) >= 1 and b"GPP_WINDOW_GENERAL" in buf.value
        yield
    finally:
        lib.gpp_set_path_override(b"GPP_WINDOW_GENERAL", None)


def is_fused(T, length, before):
    """the library's path selection (gridpp_amd/csrc/window.hip, include/gridpp_hip.h: GPP_WINDOW_FUSED_SPAN)"""
    back = min(length - 1 if before else length // 2, T)
    ahead = 0 if before else min(length // 2, T)
    return back + ((ahead + 3) & ~3) <= SPAN


def content(kind, Y, T, seed):
    rng = np.random.default_rng(seed)
    a = rng.gamma(0.7, 3.0, (Y, T)).astype(np.float32)
    if kind == "sprinkled":
        u = rng.random((Y, T))
        a[u < 0.10] = np.nan
        a[(u >= 0.10) & (u < 0.13)] = np.inf
        a[(u >= 0.13) & (u < 0.16)] = -np.inf
    elif kind == "nan_at_0":
        a[::2, 0] = np.nan
        a[1::3, :min(T, 3)] = np.nan
        a[rng.random((Y, T)) < 0.05] = np.nan
    elif kind == "all_nan_row":
        a[::2, :] = np.nan
    elif kind == "mixed_magnitude":
        a = (10.0 ** rng.uniform(-3, 4, (Y, T))).astype(np.float32)
        a[rng.random((Y, T)) < 0.03] = np.nan
    else:
        assert kind == "full"
    return a


def build_cases():
    """(Y, T, length, before, keep_missing, missing_edges, content): about a hundred, each boundary at least once on each path"""
    cases = []

    def add(Y, T, length, before, flags, kind):
        if length % 2 == 0 and not before:
            return
        case = (Y, T, length, before, flags[0], flags[1], kind)
        if case not in cases:
            cases.append(case)

    lengths_of = lambda T: (1, 2, 4, 3, 5, T, T + 2, 1001, FUSED_CENTRED, FUSED_CENTRED + 2, FUSED_BEFORE, FUSED_BEFORE + 2)   # noqa: E731
    i = 0
    for Y in YS:                      # every shape, the other choices cycling
        for T in TS:
            L = lengths_of(T)
            length, before = L[i % len(L)], i % 2 == 0
            if length % 2 == 0:
                before = True
            add(Y, T, length, before, FLAGS[i % 4], CONTENTS[i % 5])
            i += 1
    for Y, T in ((ROWS + 1, 2 * COLS + 3), (ROWS, COLS), (2 * ROWS + 3, COLS + 1)):   # every length, before and centred where the length allows
        for length in lengths_of(T):
            for before in (True, False):
                add(Y, T, length, before, FLAGS[i % 4], CONTENTS[1 + i % 4])
                i += 1
    for flags in FLAGS:               # every flag combination, both window forms, on both sides of the fused span
        for before in (True, False):
            add(ROWS + 1, 2 * COLS + 3, 5, before, flags, "sprinkled")
            add(ROWS - 1, 2 * COLS + 3, 2 * COLS + 3, before, flags, "sprinkled")
    for kind in CONTENTS:             # every content, at the largest fused span and just beyond it
        add(2 * ROWS + 3, 2 * COLS + 3, FUSED_CENTRED, False, FLAGS[0], kind)
        add(2 * ROWS + 3, 2 * COLS + 3, FUSED_BEFORE, True, FLAGS[3], kind)
        add(ROWS, 2 * COLS + 3, FUSED_CENTRED + 2, False, FLAGS[1], kind)
        add(ROWS, COLS, 3, False, FLAGS[2], kind)
    return cases


CASES = build_cases()


def case_id(c):
    return "Y%d_T%d_len%d_%s_keep%d_edges%d_%s" % (c[0], c[1], c[2], "before" if c[3] else "centred", c[4], c[5], c[6])


def test_the_case_list_hits_every_boundary_on_each_path():
    assert 80 <= len(CASES) <= 140
    fused = [c for c in CASES if is_fused(c[1], c[2], c[3])]
    general = [c for c in CASES if not is_fused(c[1], c[2], c[3])]
    assert len(fused) >= 40 and len(general) >= 15
    assert {c[0] for c in CASES} == set(YS) and {c[1] for c in CASES} == set(TS)
    assert {c[0] for c in fused} == set(YS) and {c[1] for c in fused} == set(TS)
    assert {(c[4], c[5], c[3]) for c in fused} == {(k, e, b) for k, e in FLAGS for b in (False, True)}
    assert {(c[4], c[5], c[3]) for c in general} == {(k, e, b) for k, e in FLAGS for b in (False, True)}
    assert {c[6] for c in fused} == set(CONTENTS) and {c[6] for c in general} == set(CONTENTS)
    T = 2 * COLS + 3
    assert is_fused(T, FUSED_CENTRED, False) and not is_fused(T, FUSED_CENTRED + 2, False)
    assert is_fused(T, FUSED_BEFORE, True) and not is_fused(T, FUSED_BEFORE + 2, True)
    assert is_fused(4, 1001, False) and not is_fused(T, 1001, False)   # a long window over a short row is clamped to the row
    for length in (1, 2, 4, 3, 5, 1001, FUSED_CENTRED, FUSED_CENTRED + 2, FUSED_BEFORE, FUSED_BEFORE + 2):
        assert any(c[2] == length for c in CASES)
    assert any(c[2] == c[1] for c in CASES) and any(c[2] == c[1] + 2 for c in CASES)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("case", ARRAY_CASES, ids=[c["id"] for c in ARRAY_CASES])
def test_known_answers_through_the_c_abi(gridpp, case, mem):
    """every known answer of the reference's tests/test_window.py that computes something, from host arrays and from HBM"""
    a = np.ascontiguousarray(R.case_array(case), dtype=np.float32)
    want = np.array(R._nan(case["expected"]), dtype=np.float64)
    args = (case["length"], R.STATISTIC[case["statistic"]], int(case["before"]), int(case["keep_missing"]), int(case["missing_edges"]))
    lib = _capi.lib()
    if mem == "host":
        out = np.full(a.shape, -7, np.float32)
        assert lib.gpp_window(C.c_void_p(a.ctypes.data), a.shape[0], a.shape[1], *args, C.c_void_p(out.ctypes.data), _capi.MEM_HOST) == _capi.GPP_OK
    else:
        import torch
        d = torch.from_numpy(a).cuda()
        o = torch.full(a.shape, -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert lib.gpp_window(C.c_void_p(d.data_ptr()), a.shape[0], a.shape[1], *args, C.c_void_p(o.data_ptr()), _capi.MEM_DEVICE) == _capi.GPP_OK
        out = o.cpu().numpy()
    np.testing.assert_array_equal(out, want)


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_bit_equal_to_the_restatement_on_both_paths(gridpp, case):
    import torch
    Y, T, length, before, keep, edges, kind = case
    a = content(kind, Y, T, seed=Y * 1000 + T * 7 + length)
    d = torch.from_numpy(a).cuda()
    fused = is_fused(T, length, before)
    for statistic in EXACT:
        want = R.window(a, length, statistic, before, keep, edges)
        got = gridpp.window(a, length, statistic, before, keep, edges)            # host arrays, the path the library picks
        assert isinstance(got, np.ndarray) and got.dtype == np.float32
        R.same_bits(got, want)
        if fused:                                                                 # HBM tensors, the general path forced
            with general_path():
                other = gridpp.window(d, length, statistic, before, keep, edges)
            assert isinstance(other, torch.Tensor) and other.is_cuda and other.dtype == torch.float32
            R.same_bits(other.cpu().numpy(), got)
        else:                                                                     # (already the general path: the device path on it)
            R.same_bits(gridpp.window(d, length, statistic, before, keep, edges).cpu().numpy(), got)
    got = gridpp.window(a, length, R.RandomChoice, before, keep, edges)
    R.check_random_choice(got, a, length, before, keep, edges)
    with general_path():
        R.check_random_choice(gridpp.window(a, length, R.RandomChoice, before, keep, edges), a, length, before, keep, edges)


def test_random_choice_draws_more_than_one_member(gridpp):
    """a hash per output, not "the first valid value": over many windows every position of the window is drawn"""
    a = np.tile(np.arange(5, dtype=np.float32), (4 * ROWS, 8))   # rows 0 1 2 3 4 0 1 ... : a window of 5 holds each value once
    got = gridpp.window(a, 5, R.RandomChoice, False, False, False)
    R.check_random_choice(got, a, 5, False, False, False)
    inner = got[:, 2:-2]
    assert {float(v) for v in np.unique(inner)} == {0.0, 1.0, 2.0, 3.0, 4.0}


@pytest.mark.parametrize("T", [2 * COLS, 2 * COLS + 4, 3 * COLS])
def test_whole_16_byte_groups_over_several_chunks(gridpp, T):
    """T a multiple of 4 from aligned arrays: the 16-byte accesses, over rows of more than one chunk (TS holds one such T, a single
    chunk).  Centred windows start the walk one step early (the chunk in front of column 0) and the ring wraps from the second chunk on;
    the lengths are the shortest, the one whose lead is a whole group, and the largest fused one of each window form and the next."""
    import torch
    Y = ROWS + 1
    a = content("sprinkled", Y, T, seed=T)
    d = torch.from_numpy(a).cuda()
    assert d.data_ptr() % 16 == 0 and T % 4 == 0
    for length, before in ((3, False), (9, False), (FUSED_CENTRED, False), (FUSED_CENTRED + 2, False), (FUSED_BEFORE, True), (FUSED_BEFORE + 2, True)):
        for statistic in EXACT:
            want = R.window(a, length, statistic, before, False, False)
            R.same_bits(gridpp.window(d, length, statistic, before, False, False).cpu().numpy(), want)
            R.same_bits(gridpp.window(a, length, statistic, before, False, False), want)
            with general_path():
                R.same_bits(gridpp.window(d, length, statistic, before, False, False).cpu().numpy(), want)
        R.same_bits(gridpp.window(d, length, R.Mean, before, True, True).cpu().numpy(), R.window(a, length, R.Mean, before, True, True))


def test_unaligned_device_tensor_takes_the_scalar_accesses(gridpp):
    """T is a multiple of 4 but the tensor starts 4 bytes past a 16-byte boundary: the kernels may not use 16-byte accesses"""
    import torch
    Y, T = ROWS + 1, 2 * COLS
    a = content("sprinkled", Y, T, seed=5)
    buf = torch.zeros(Y * T + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(Y, T)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    for statistic, length, before in ((R.Sum, 5, False), (R.Mean, 24, True), (R.Max, 7, False), (R.Sum, 101, False), (R.Median, 35, True)):
        got = gridpp.window(view, length, statistic, before, False, True)
        R.same_bits(got.cpu().numpy(), R.window(a, length, statistic, before, False, True))


def test_float64_host_array_goes_up_as_it_is(gridpp):
    """2^20 float64 values: handed over with GPP_HOST_F64 and rounded on the device == the float32 path on the rounded input"""
    rng = np.random.default_rng(64)
    a64 = rng.gamma(0.7, 3.0, (1 << 14, 64)) * (1 + 1e-9)
    a64[rng.random(a64.shape) < 0.02] = np.nan
    assert a64.dtype == np.float64 and a64.size >= 1 << 20 and gridpp._wants_f64(a64)
    a32 = a64.astype(np.float32)
    assert np.any(a32.astype(np.float64) != a64)   # (the rounding changes values: the comparison is not vacuous)
    for statistic, length, before in ((R.Sum, 24, True), (R.Max, 7, False)):
        got = gridpp.window(a64, length, statistic, before)
        assert got.dtype == np.float32 and got.shape == a64.shape
        R.same_bits(got, gridpp.window(a32, length, statistic, before))
    R.same_bits(got[-3 * ROWS:], R.window(a32[-3 * ROWS:], 7, R.Max, False))
