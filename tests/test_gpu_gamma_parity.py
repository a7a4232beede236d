"""GPU: k_gamma_inv and k_gamma_transform against tests/golden/gamma_cases.npz (mpmath, every case of it in every test that loads it) --
as float32 host arrays, as float64 host arrays (through the public call, which rounds small arrays on the host, and through the C-ABI
with GPP_HOST_F64, which rounds on the device) and as torch CUDA tensors whose result stays on the device; at n = 1, 2, 3, 5, one
workgroup +- 1, the golden file's own length and one value more than the capped grid covers in one stride (the golden cases tiled to fill
them); through views that start 4 bytes off a 16-byte boundary; as 1-, 2- and 3-D shapes; against the host scalar forms on the same
inputs (one source, two compilers); the three gamma_inv errors through the status word; and backward(forward(x)) = x.

Tolerance: the rule of tests/gamma_ref.py."""
import ctypes as C

import numpy as np
import pytest

from tests import gamma_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
NOT_F32 = 1 + 2.0 ** -30   # a float64 factor that leaves no float32 value a float32 value, and rounds back to it


@pytest.fixture(scope="module")
def amd():
    import gridpp_amd
    assert gridpp_amd.device_count() > 0
    return gridpp_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def capi():
    from gridpp_amd import _capi
    return _capi


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def lengths(capi, golden_n):
    block, stride = capi.GAMMA_BLOCK, capi.GAMMA_BLOCK * capi.GAMMA_MAX_BLOCKS   # the kernel's own constants
    return [1, 2, 3, 5, block - 1, block, block + 1, golden_n, stride + 1]


def kinds(torch):
    """how the inputs of a call are handed over -> (name, convert)"""
    return [("float32", lambda a: a.copy()), ("float64", lambda a: a.astype(np.float64)), ("tensor", lambda a: torch.from_numpy(a.copy()).cuda())]


def check_kind(torch, name, got, n):
    if name == "tensor":
        assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (n,)
    else:
        assert isinstance(got, np.ndarray) and got.dtype == F and got.shape == (n,)


# ---- the golden file through both kernels --------------------------------------------------------------------------------------------------
def test_gamma_inv_golden(amd, torch, capi):
    g = R.golden()
    lib = capi.lib()
    for n in lengths(capi, len(g.gi_want)):
        level, shape, scale, want = (R.tile(a, n) for a in (g.gi_level, g.gi_shape, g.gi_scale, g.gi_want))
        for name, conv in kinds(torch):
            got = amd.gamma_inv(conv(level), conv(shape), conv(scale))
            check_kind(torch, name, got, n)
            idx = R.mismatches(host(got), want)
            assert len(idx) == 0, "%s n=%d: %s" % (name, n, R.report(idx, host(got), want, level, shape, scale))
        # GPP_HOST_F64: doubles that are no float32 values, rounded on the device as the first operation
        wide = [a.astype(np.float64) * NOT_F32 for a in (level, shape, scale)]
        assert all((w.astype(F) == a).all() or np.isnan(a).any() for w, a in zip(wide, (level, shape, scale)))
        out = np.full(n, 7, F)
        assert lib.gpp_gamma_inv(ptr(wide[0]), ptr(wide[1]), ptr(wide[2]), n, ptr(out), capi.MEM_HOST | capi.HOST_F64) == 0, lib.gpp_last_error()
        idx = R.mismatches(out, want)
        assert len(idx) == 0, "GPP_HOST_F64 n=%d: %s" % (n, R.report(idx, out, want, level, shape, scale))


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_transform_golden(amd, torch, capi, direction):
    g = R.golden()
    lib = capi.lib()
    backward = direction == "backward"
    sets = [(p, v, w, ()) for p, v, w in g.backward_sets()] if backward else list(g.forward_sets())
    assert sum(len(s[1]) for s in sets) == len(g.bw_in if backward else g.fw_in)
    for params, values, want, neighbours in sets:
        t = amd.Gamma(*params)
        for n in lengths(capi, len(values)):
            v, w, alt = R.tile(values, n), R.tile(want, n), [R.tile(a, n) for a in neighbours]
            for name, conv in kinds(torch):
                got = getattr(t, direction)(conv(v))
                check_kind(torch, name, got, n)
                idx = R.mismatches(host(got), w, alt)
                assert len(idx) == 0, "%s %s %s n=%d: %s" % (direction, params, name, n, R.report(idx, host(got), w, v))
            wide, out = v.astype(np.float64) * NOT_F32, np.full(n, 7, F)
            assert lib.gpp_gamma_transform(ptr(wide), n, int(backward), F(params[0]), F(params[1]), F(params[2]), ptr(out), capi.MEM_HOST | capi.HOST_F64) == 0
            idx = R.mismatches(out, w, alt)
            assert len(idx) == 0, "%s %s GPP_HOST_F64 n=%d: %s" % (direction, params, n, R.report(idx, out, w, v))


def test_big_float64_host_arrays_take_the_device_rounding(amd):
    """float64 numpy arrays of 2^20 values and more are handed over as they are (GPP_HOST_F64)"""
    g = R.golden()
    n = (1 << 20) + 3
    level, shape, scale, want = (R.tile(a, n) for a in (g.gi_level, g.gi_shape, g.gi_scale, g.gi_want))
    got = amd.gamma_inv(*[a.astype(np.float64) * NOT_F32 for a in (level, shape, scale)])
    assert isinstance(got, np.ndarray) and got.dtype == F
    idx = R.mismatches(got, want)
    assert len(idx) == 0, R.report(idx, got, want, level, shape, scale)
    params, values, want, neighbours = next(g.forward_sets())
    v = R.tile(values, n).astype(np.float64) * NOT_F32
    got = amd.Gamma(*params).forward(v)
    idx = R.mismatches(got, R.tile(want, n), [R.tile(a, n) for a in neighbours])
    assert len(idx) == 0, R.report(idx, got, R.tile(want, n), v)


# ---- alignment and shapes ---------------------------------------------------------------------------------------------------------------
def test_views_four_bytes_off_a_16_byte_boundary(amd, torch, capi):
    """inputs AND output start at element 1 of an aligned allocation: the bits of the aligned call"""
    g = R.golden()
    lib = capi.lib()
    n = len(g.gi_want)
    dev = [torch.from_numpy(np.concatenate([[F(0.5)], a])).cuda() for a in (g.gi_level, g.gi_shape, g.gi_scale)]
    assert all(d.data_ptr() % 16 == 0 and d[1:].data_ptr() % 16 == 4 for d in dev)
    aligned = amd.gamma_inv(*[d[1:].clone() for d in dev])
    idx = R.mismatches(host(aligned), g.gi_want)
    assert len(idx) == 0, R.report(idx, host(aligned), g.gi_want, g.gi_level, g.gi_shape, g.gi_scale)
    sliced = amd.gamma_inv(*[d[1:] for d in dev])
    assert torch.equal(sliced.view(torch.int32), aligned.view(torch.int32))
    out = torch.full((n + 2,), 7.0, device="cuda")
    torch.cuda.synchronize()
    assert lib.gpp_gamma_inv(*[C.c_void_p(d[1:].data_ptr()) for d in dev], n, C.c_void_p(out[1:].data_ptr()), capi.MEM_DEVICE) == 0
    assert torch.equal(out[1:n + 1].view(torch.int32), aligned.view(torch.int32)) and out[0] == 7 and out[n + 1] == 7
    for direction, sets in (("forward", list(g.forward_sets())), ("backward", list(g.backward_sets()))):
        for s in sets:
            params, values = s[0], s[1]
            t, m = amd.Gamma(*params), len(values)
            d = torch.from_numpy(np.concatenate([[F(1)], values])).cuda()
            aligned = getattr(t, direction)(d[1:].clone())
            assert torch.equal(getattr(t, direction)(d[1:]).view(torch.int32), aligned.view(torch.int32))
            out = torch.full((m + 2,), 7.0, device="cuda")
            torch.cuda.synchronize()
            assert lib.gpp_gamma_transform(C.c_void_p(d[1:].data_ptr()), m, int(direction == "backward"), F(params[0]), F(params[1]), F(params[2]),
                                           C.c_void_p(out[1:].data_ptr()), capi.MEM_DEVICE) == 0
            assert torch.equal(out[1:m + 1].view(torch.int32), aligned.view(torch.int32)) and out[0] == 7 and out[m + 1] == 7
            want = s[2]
            idx = R.mismatches(host(aligned), want, s[3] if direction == "forward" else ())
            assert len(idx) == 0, "%s %s: %s" % (direction, params, R.report(idx, host(aligned), want, values))


def test_one_two_and_three_dimensions(amd, torch):
    g = R.golden()
    for direction, sets in (("forward", list(g.forward_sets())), ("backward", list(g.backward_sets()))):
        for s in sets:
            params, values, want = s[0], s[1], s[2]
            alt = s[3] if direction == "forward" else ()
            call = getattr(amd.Gamma(*params), direction)
            n = len(values) - len(values) % 12
            flat = call(values[:n].copy())
            idx = R.mismatches(flat, want[:n], [a[:n] for a in alt])
            assert len(idx) == 0, "%s %s: %s" % (direction, params, R.report(idx, flat, want[:n], values[:n]))
            rest = call(values[n:].copy())   # the cases that do not fill the shapes are compared too
            idx = R.mismatches(rest, want[n:], [a[n:] for a in alt])
            assert len(idx) == 0, "%s %s: %s" % (direction, params, R.report(idx, rest, want[n:], values[n:]))
            for shape in ((n,), (n // 4, 4), (3, n // 12, 4), (1, 1, n), (n, 1)):
                for given in (values[:n].reshape(shape).copy(), values[:n].reshape(shape).tolist(), values[:n].reshape(shape).astype(np.float64),
                              torch.from_numpy(values[:n].reshape(shape).copy()).cuda()):
                    got = call(given)
                    assert tuple(got.shape) == shape and (got.is_cuda if torch.is_tensor(given) else isinstance(got, np.ndarray) and got.dtype == F)
                    np.testing.assert_array_equal(host(got).ravel().view(np.uint32), flat.view(np.uint32))
    with pytest.raises(RuntimeError, match="got 4"):
        amd.Gamma(1, 2).forward(np.zeros((2, 2, 2, 2)))
    assert tuple(amd.Gamma(1, 2).forward(torch.zeros((0, 1), device="cuda")).shape) == (0, 0)


# ---- one source, two compilers ------------------------------------------------------------------------------------------------------------
def test_kernel_against_the_host_scalar_forms(amd, capi):
    g = R.golden()
    lib = capi.lib()
    res = C.c_float()

    def scalar(entry, *args):
        assert entry(*args, C.byref(res)) == 0
        return res.value
    got = amd.gamma_inv(g.gi_level.copy(), g.gi_shape.copy(), g.gi_scale.copy())
    want = np.array([scalar(lib.gpp_gamma_inv_scalar, *c) for c in zip(g.gi_level, g.gi_shape, g.gi_scale)], F)
    idx = R.mismatches(got, want)
    assert len(idx) == 0, R.report(idx, got, want, g.gi_level, g.gi_shape, g.gi_scale)
    for direction, sets in ((0, list(g.forward_sets())), (1, list(g.backward_sets()))):
        for s in sets:
            params, values = s[0], s[1]
            t = amd.Gamma(*params)
            got = t.backward(values.copy()) if direction else t.forward(values.copy())
            want = np.array([scalar(lib.gpp_gamma_transform_scalar, v, direction, F(params[0]), F(params[1]), F(params[2])) for v in values], F)
            # forward: the two compilers' cdf may fall on either side of a float32 rounding boundary, as against the golden values
            alt = (s[3][0], s[3][1], s[2]) if direction == 0 else ()
            idx = R.mismatches(got, want, alt)
            assert len(idx) == 0, "%s %s: %s" % (direction, params, R.report(idx, got, want, values))


# ---- the errors of gamma_inv: the status word ----------------------------------------------------------------------------------------------
def test_gamma_inv_reports_the_lowest_offending_index(amd, torch, capi):
    block, n = capi.GAMMA_BLOCK, capi.GAMMA_BLOCK * capi.GAMMA_MAX_BLOCKS + 1
    level, shape, scale = np.full(n, 0.5, F), np.full(n, 2, F), np.full(n, 3, F)

    def expect(text, lv, a, s):
        for conv in (lambda x: x.copy(), lambda x: x.astype(np.float64), lambda x: torch.from_numpy(x.copy()).cuda()):
            with pytest.raises(ValueError) as e:
                amd.gamma_inv(conv(lv), conv(a), conv(s))
            assert str(e.value) == text
    # an invalid level in the last element (the one the second stride of workgroup 0 computes)
    lv = level.copy()
    lv[-1] = 1.5
    expect("Invalid level '1.5'. Levels must be on the interval [0, 1].", lv, shape, scale)
    # invalid elements in two different workgroups: the lower index is reported, whatever its kind
    lv, a, s = level.copy(), shape.copy(), scale.copy()
    a[block + 44], lv[7 * block + 3], s[n - 2] = -2.25, np.nan, 0
    expect("Invalid shape '-2.25'. Shapes must be > 0.", lv, a, s)
    lv[block + 43] = -0.125
    expect("Invalid level '-0.125'. Levels must be on the interval [0, 1].", lv, a, s)
    # an invalid shape and level in one element: the level wins; then the shape before the scale
    lv, a, s = level[:5].copy(), shape[:5].copy(), scale[:5].copy()
    lv[3], a[3], s[3] = 1.25, np.inf, -1
    expect("Invalid level '1.25'. Levels must be on the interval [0, 1].", lv, a, s)
    lv[3] = 1
    expect("Invalid shape 'inf'. Shapes must be > 0.", lv, a, s)
    a[3] = 1
    expect("Invalid scale '-1'. Scale must be > 0.", lv, a, s)
    # GPP_HOST_F64: the value reported is the float32 the kernel saw
    wide = [x.astype(np.float64) for x in (lv, a, s)]
    wide[2][3] = -1 - 2.0 ** -40
    out = np.zeros(5, F)
    lib = capi.lib()
    assert lib.gpp_gamma_inv(ptr(wide[0]), ptr(wide[1]), ptr(wide[2]), 5, ptr(out), capi.MEM_HOST | capi.HOST_F64) == capi.GPP_EINVAL
    assert lib.gpp_last_error().decode() == "Invalid scale '-1'. Scale must be > 0."
    # and the next call starts from a clean status word
    s[3] = 2
    assert amd.gamma_inv(lv, a, s)[3] == np.inf
    assert len(R.mismatches(amd.gamma_inv(level[:5], shape[:5], scale[:5]), np.full(5, amd.gamma_inv(0.5, 2.0, 3.0), F))) == 0


# ---- the round trip ------------------------------------------------------------------------------------------------------------------------
def test_backward_undoes_forward(amd, torch):
    """tests/test_transform.py:82-86 of the reference asks 5 decimals of backward(forward(x)) at 0 and 1.99 for Gamma(1, 2, 0.01); here 1e-5
    absolute over [0, 6].  Why 6: the float32 stores of the cdf (twice) and of the normal score put at most about 1e-7 of absolute error on
    the cdf; the gamma quantile turns that into 1e-7 / pdf(x) = 2e-7 exp(x / 2), which is 4e-6 at x = 6 and passes 1e-5 near x = 7.8."""
    t = amd.Gamma(1, 2, 0.01)
    x = np.linspace(0, 6, 4801).astype(F)
    for given in (x.copy(), torch.from_numpy(x.copy()).cuda()):
        back = host(t.backward(t.forward(given)))
        assert np.max(np.abs(back.astype(np.float64) - x)) <= 1e-5, np.max(np.abs(back.astype(np.float64) - x))
