"""GPU: every weather diagnostic and every value transform in both directions against the numpy restatement (tests/pointwise_ref.py).

Lengths around every edge of k_pointwise: one to five values (the tail launch alone), the 4-value step, one workgroup, and, with
P = GPP_POINTWISE_BLOCK * GPP_POINTWISE_MAX_BLOCKS * 4 values per pass of the whole grid, P - 1, P and P + 5 (a second grid-stride step
and a tail, 8 MB per array).  Device tensors whose inputs, each alone and all but each, have lost their 16-byte alignment must give the
bits of the aligned call.  Non-contiguous and float64 tensors, lists, float32 and float64 host arrays (GPP_HOST_F64 above 2^20 values).
sea_level_pressure reports the lowest offending index.

Tolerance (the issue's): bit for bit for Identity, wind_speed and relative_humidity; 1e-5 relative for the rest, NaN matching NaN,
infinities by sign, -0.0 equal to 0; BoxCox.forward near an input of 1 on the power it computed.  The count of values that are not
bit-identical to the restatement is printed for every function (recorded in DESIGN.md 4.10, not a criterion).

The restatement of each function is computed once, on the longest input; every shorter case compares with a prefix of it."""
import ctypes as C

import numpy as np
import pytest

from tests import pointwise_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = list(R.DIAGNOSTICS)
TRANSFORMS = R.transforms()
TIDS = [t[0] for t in TRANSFORMS]


@pytest.fixture(scope="module")
def gridpp():
    import gridpp
    assert gridpp.implementation == "gridpp_amd" and gridpp.device_count() > 0
    return gridpp


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def P():
    from gridpp_amd import _capi
    return _capi.POINTWISE_BLOCK * _capi.POINTWISE_MAX_BLOCKS * 4


def lengths(P):
    return [1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, P - 1, P, P + 5]


_cache = {}


def diag_case(name, P):
    """-> (inputs, want) of P + 5 seeded values, nothing that makes sea_level_pressure throw; computed once"""
    if name not in _cache:
        args = R.seeded_inputs(name, P + 5, offenders=False)
        want = getattr(R, name)(*args)
        if name == "sea_level_pressure":
            assert not want[1].any()
            want = want[0]
        for a in args + [want]:
            a.setflags(write=False)
        _cache[name] = (args, want)
    return _cache[name]


def transform_case(tid, direction, P):
    key = (tid, direction)
    if key not in _cache:
        cls, params = next((c, p) for t, c, p in TRANSFORMS if t == tid)
        values = R.seeded_values(direction, P + 5)
        want = getattr(getattr(R, cls)(*params), direction)(values)
        values.setflags(write=False), want.setflags(write=False)
        _cache[key] = (values, want)
    return _cache[key]


def diag_bad(name, got, want):
    return R.mismatches(got, want, 0 if name in R.EXACT else R.RTOL)


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


# ---- lengths ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_diagnostic_lengths(gridpp, torch, P, name):
    args, want = diag_case(name, P)
    dev = [torch.tensor(a, device="cuda") for a in args]
    for n in lengths(P):
        out = getattr(gridpp, name)(*[d[:n] for d in dev])
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n,)
        got = host(out)
        bad = diag_bad(name, got, want[:n])
        assert bad.size == 0, (name, n, [(int(i), [a[i] for a in args], got[i], want[i]) for i in bad[:5]])
    print("%s: %d of %d values not bit-identical to the restatement on the GPU" % (name, R.bit_differences(got, want), P + 5))


@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("tid,cls,params", TRANSFORMS, ids=TIDS)
def test_transform_lengths(gridpp, torch, P, tid, cls, params, direction):
    values, want = transform_case(tid, direction, P)
    dev = torch.tensor(values, device="cuda")
    fn = getattr(getattr(gridpp, cls)(*params), direction)
    for n in lengths(P):
        out = fn(dev[:n])
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n,)
        got = host(out)
        bad = R.transform_mismatches(tid, direction, values[:n], got, want[:n])
        assert bad.size == 0, (tid, direction, n, [(int(i), values[i], got[i], want[i]) for i in bad[:5]])
    print("%s.%s: %d of %d values not bit-identical to the restatement on the GPU" % (tid, direction, R.bit_differences(got, want), P + 5))


# ---- alignment ----------------------------------------------------------------------------------------------------------------------------
def shifted(torch, a, k):
    """a copy of the device tensor a that starts k floats behind a 16-byte boundary"""
    buf = torch.empty(a.numel() + 4, dtype=a.dtype, device=a.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[k:k + a.numel()]
    view.copy_(a)
    assert view.data_ptr() % 16 == (4 * k) % 16
    return view


@pytest.mark.parametrize("name", NAMES)
def test_unaligned_inputs_give_the_bits_of_the_aligned_call(gridpp, torch, P, name):
    args, want = diag_case(name, P)
    n = 1025
    dev = [torch.from_numpy(a[:n].copy()).cuda() for a in args]
    assert all(d.data_ptr() % 16 == 0 for d in dev)
    aligned = getattr(gridpp, name)(*dev)
    assert diag_bad(name, host(aligned), want[:n]).size == 0
    for k in (1, 2, 3):
        for i in range(len(dev)):
            only = [shifted(torch, d, k) if j == i else d for j, d in enumerate(dev)]       # input i alone
            others = [shifted(torch, d, k) if j != i else d for j, d in enumerate(dev)]     # every input but i
            for variant in (only, others):
                out = getattr(gridpp, name)(*variant)
                assert torch.equal(out.view(torch.int32), aligned.view(torch.int32)), (name, k, i)
        sliced = getattr(gridpp, name)(*[d[k:] for d in dev])                               # the issue's [1:], [2:], [3:]
        assert torch.equal(sliced.view(torch.int32), aligned[k:].view(torch.int32)), (name, k)


@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("tid,cls,params", TRANSFORMS, ids=TIDS)
def test_unaligned_transform_input_and_output(gridpp, torch, P, tid, cls, params, direction):
    """the input through the Python surface, the output through the C-ABI (the surface allocates its results aligned)"""
    from gridpp_amd import _capi
    values, want = transform_case(tid, direction, P)
    n = 1025
    dev = torch.from_numpy(values[:n].copy()).cuda()
    t = getattr(gridpp, cls)(*params)
    aligned = getattr(t, direction)(dev)
    assert R.transform_mismatches(tid, direction, values[:n], host(aligned), want[:n]).size == 0
    p0, p1 = t._params()
    for k in (1, 2, 3):
        assert torch.equal(getattr(t, direction)(shifted(torch, dev, k)).view(torch.int32), aligned.view(torch.int32))
        assert torch.equal(getattr(t, direction)(dev[k:]).view(torch.int32), aligned[k:].view(torch.int32))
        buf = torch.full((n + 8,), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rc = _capi.lib().gpp_transform(C.c_void_p(dev.data_ptr()), n, t._kind, int(direction == "backward"), p0, p1, C.c_void_p(buf.data_ptr() + 4 * k),
                                       _capi.MEM_DEVICE)
        assert rc == _capi.GPP_OK
        assert torch.equal(buf[k:k + n].view(torch.int32), aligned.view(torch.int32))
        assert bool((buf[:k] == 7).all()) and bool((buf[k + n:] == 7).all())      # nothing outside the n values


# ---- other tensors and host arrays ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_noncontiguous_and_float64_tensors(gridpp, torch, P, name):
    args, want = diag_case(name, P)
    n = 1025
    dev = [torch.from_numpy(a[:2 * n].copy()).cuda() for a in args]
    out = getattr(gridpp, name)(*[d[::2] for d in dev])
    assert not dev[0][::2].is_contiguous()
    assert diag_bad(name, host(out), want[:2 * n:2]).size == 0
    out = getattr(gridpp, name)(*[d[:n].double() for d in dev])
    assert out.dtype == torch.float32 and diag_bad(name, host(out), want[:n]).size == 0


@pytest.mark.parametrize("name", NAMES)
def test_host_arrays(gridpp, torch, P, name):
    args, want = diag_case(name, P)
    fn = getattr(gridpp, name)
    for n in (5, 1025):
        for conv in (lambda a: a[:n].tolist(), lambda a: a[:n].copy(), lambda a: a[:n].astype(np.float64)):
            out = fn(*[conv(a) for a in args])
            assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == (n,)
            assert diag_bad(name, out, want[:n]).size == 0, (name, n)
    # float64 arrays of 2^20 + 3 values that are no float32 values: handed over as they are (GPP_HOST_F64), rounded on the device
    n = (1 << 20) + 3
    wide = [a[:n].astype(np.float64) * (1 + 2.0 ** -30) for a in args]
    assert any((w != w.astype(F)).any() for w in wide)
    want64 = getattr(R, name)(*wide)
    want64 = want64[0] if name == "sea_level_pressure" else want64
    out = fn(*wide)
    assert out.dtype == F and diag_bad(name, out, want64).size == 0, name
    # one big float64 input beside a big float32 one: the float32 path, every input converted on the host
    mixed = [w.astype(F) if i == 1 else w for i, w in enumerate(wide)]
    want_mixed = getattr(R, name)(*mixed)
    want_mixed = want_mixed[0] if name == "sea_level_pressure" else want_mixed
    assert diag_bad(name, fn(*mixed), want_mixed).size == 0, name


@pytest.mark.parametrize("tid,cls,params", TRANSFORMS, ids=TIDS)
def test_transform_shapes_and_host_arrays(gridpp, torch, P, tid, cls, params):
    t, r = getattr(gridpp, cls)(*params), getattr(R, cls)(*params)
    for direction in ("forward", "backward"):
        values, want = transform_case(tid, direction, P)
        fn = getattr(t, direction)
        for shape in ((3, 3, 3), (257, 5), (1025,)):
            n = int(np.prod(shape))
            v = values[:n].reshape(shape)
            for given in (v.copy(), v.tolist(), v.astype(np.float64), torch.from_numpy(v.copy()).cuda(), torch.from_numpy(v.copy()).cuda().double()):
                out = fn(given)
                assert tuple(out.shape) == shape and (out.is_cuda if hasattr(given, "is_cuda") else isinstance(out, np.ndarray))
                assert R.transform_mismatches(tid, direction, v, host(out), want[:n]).size == 0, (tid, direction, shape)
        # a non-contiguous tensor
        d = torch.from_numpy(values[:2 * 257 * 5].reshape(257, 10).copy()).cuda()[:, ::2]
        assert R.transform_mismatches(tid, direction, host(d), host(fn(d)), getattr(r, direction)(host(d))).size == 0
        # float64 above 2^20 values: GPP_HOST_F64
        n = (1 << 20) + 3
        wide = values[:n].astype(np.float64) * (1 + 2.0 ** -30)
        assert R.transform_mismatches(tid, direction, wide, fn(wide), getattr(r, direction)(wide)).size == 0
        # the empty shapes, on the device too
        for shape, want_shape in (((0, 1), (0, 0)), ((2, 0), (2, 0)), ((3, 3, 0), (3, 3, 0)), ((0, 3, 3), (0, 0, 0)), ((0,), (0,))):
            assert fn(np.zeros(shape)).shape == want_shape
            out = fn(torch.zeros(shape, device="cuda"))
            assert out.is_cuda and tuple(out.shape) == want_shape


def test_base_class_vectors_are_minus_one(gridpp, torch):
    assert np.all(gridpp.Transform().forward(np.zeros((3, 4))) == -1)
    out = gridpp.Transform().backward(torch.zeros((3, 4, 5), device="cuda"))
    assert out.is_cuda and tuple(out.shape) == (3, 4, 5) and bool((out == -1).all())


# ---- errors out of the kernel ---------------------------------------------------------------------------------------------------------------
def test_sea_level_pressure_reports_the_lowest_offending_index(gridpp, torch, P):
    args, want = diag_case("sea_level_pressure", P)
    n = 1025
    clean = [a[:n].copy() for a in args]
    bad = [a.copy() for a in clean]
    bad[1][1000] = np.nan      # altitude is NAN
    bad[0][17] = -1            # unphysical values in input
    bad[2][900] = np.nan       # temperature is NAN
    for conv in (lambda a: a, lambda a: torch.from_numpy(a).cuda()):
        with pytest.raises(RuntimeError) as e:
            gridpp.sea_level_pressure(*[conv(a) for a in bad])
        assert str(e.value) == "sea_level_pressure: unphysical values in input"
        out = gridpp.sea_level_pressure(*[conv(a) for a in clean])      # the status word starts afresh
        assert diag_bad("sea_level_pressure", host(out), want[:n]).size == 0
    # each kind alone, in the wide launch and in the tail (n = 1025: index 1024 is the VEC = 1 launch)
    for index, (arg, value, message) in ((1000, (1, np.inf, "altitude is NAN")), (900, (2, np.nan, "temperature is NAN")), (1024, (3, 1.5, "unphysical values in input")),
                                         (1024, (1, np.nan, "altitude is NAN"))):
        one = [a.copy() for a in clean]
        one[arg][index] = value
        with pytest.raises(RuntimeError) as e:
            gridpp.sea_level_pressure(*[torch.from_numpy(a).cuda() for a in one])
        assert str(e.value) == "sea_level_pressure: " + message
    # the C-ABI writes the values all the same, NaN at the offending elements
    from gridpp_amd import _capi
    dev = [torch.from_numpy(a).cuda() for a in bad]
    out = torch.zeros(n, device="cuda")
    torch.cuda.synchronize()
    rc = _capi.lib().gpp_sea_level_pressure(*[C.c_void_p(d.data_ptr()) for d in dev], n, C.c_void_p(out.data_ptr()), _capi.MEM_DEVICE)
    assert rc == _capi.GPP_ERUNTIME
    expected = want[:n].copy()
    expected[[17, 900, 1000]] = np.nan
    assert diag_bad("sea_level_pressure", host(out), expected).size == 0
