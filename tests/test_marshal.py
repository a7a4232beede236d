"""CPU: the argument-marshalling layer of the Python wrappers (gridpp_amd/_marshal.py) on its own -- no library, no device."""
import numpy as np
import pytest

from gridpp_amd import _capi
from gridpp_amd import _marshal as m


class FakeDeviceTensor:
    """what _is_dev looks for; any use beyond that (a synchronise of torch's stream included) is an error of the code under test"""
    is_cuda = True

    def data_ptr(self):
        raise AssertionError("the stand-in tensor must not be read")


# ---- field ----------------------------------------------------------------------------------------------------------------
def test_field_returns_the_same_buffer_when_nothing_is_to_do():
    a32, a64 = np.arange(6, dtype=np.float32).reshape(2, 3), np.arange(6, dtype=np.float64).reshape(2, 3)
    assert m.field(a32) is a32 and m.field(a32, 2) is a32 and m.field(a32, 2, "x", False) is a32
    assert m.field(a64, f64=True) is a64 and m.field(a64, 2, "x", True) is a64
    i32 = np.arange(6, dtype=np.int32).reshape(2, 3)
    assert m.field(i32, dtype=np.int32) is i32


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("make", [
    lambda: np.arange(6).reshape(2, 3),                                      # int
    lambda: np.arange(6, dtype=np.float64).reshape(2, 3),                    # float64 (converted unless the call is a float64 one)
    lambda: np.arange(6, dtype=np.float32).reshape(2, 3),                    # float32 (converted in a float64 call)
    lambda: [[0, 1, 2], [3, 4, 5]],                                          # lists
    lambda: np.asfortranarray(np.arange(6, dtype=np.float32).reshape(2, 3)),  # Fortran order
    lambda: np.arange(12, dtype=np.float32).reshape(2, 6)[:, ::2],           # a strided view
    lambda: np.arange(24, dtype=np.float64).reshape(4, 6)[::2, 1::2],        # a view strided both ways
], ids=["int", "float64", "float32", "lists", "fortran", "strided", "strided2"])
def test_field_converts_to_a_c_contiguous_array_of_the_call_dtype(make, f64):
    src = make()
    for ndim in (None, 2):
        out = m.field(src, ndim, "x", f64)
        assert isinstance(out, np.ndarray) and out.flags["C_CONTIGUOUS"]
        assert out.dtype == (np.float64 if f64 else np.float32) and out.shape == (2, 3)
        np.testing.assert_array_equal(out, np.asarray(src))


def test_field_strided_and_fortran_inputs_are_copied_not_aliased():
    base = np.arange(12, dtype=np.float32).reshape(2, 6)
    view = base[:, ::2]
    out = m.field(view, 2)
    assert out.flags["C_CONTIGUOUS"] and not np.shares_memory(out, base)
    np.testing.assert_array_equal(out, [[0, 2, 4], [6, 8, 10]])
    f = np.asfortranarray(np.arange(6, dtype=np.float32).reshape(2, 3))
    assert not np.shares_memory(m.field(f), f)


def test_field_dtype_argument_wins():
    out = m.field([[0.0, 1.9], [2.0, -1.9]], 2, "mask", dtype=np.int32)
    assert out.dtype == np.int32
    np.testing.assert_array_equal(out, [[0, 1], [2, -1]])


def test_field_none_passes_through():
    assert m.field(None) is None and m.field(None, 2, "x", True) is None


def test_field_empty_lists_take_the_rank_asked_for():
    assert m.field([], 1).shape == (0,) and m.field([], 2).shape == (0, 0) and m.field([], 3).shape == (0, 0, 0)
    assert m.field([[]], 2).shape == (1, 0)       # (already two-dimensional: numpy's shape of [[]] stays)
    assert m.field([[]], 3).shape == (0, 0, 0)
    assert m.field([], 2, f64=True).dtype == np.float64
    assert m._vec([], 1).shape == (0,) and m._vec([[]], 3).shape == (0, 0, 0)
    assert m.field([]).shape == (0,) and m.field([[]]).shape == (1, 0)    # no rank asked for: converted only


def test_field_wrong_rank_raises_the_typemap_text():
    with pytest.raises(RuntimeError) as e:
        m.field(np.zeros(3), 2, "values")
    assert str(e.value) == "values must have 2 dimensions, got 1"
    with pytest.raises(RuntimeError) as e:
        m.field(np.zeros((2, 2, 2)), 1)
    assert str(e.value) == "array must have 1 dimensions, got 3"
    with pytest.raises(RuntimeError) as e:
        m.field(np.zeros((0, 2, 2)), 2, "h", True)      # empty, but of too many dimensions
    assert str(e.value) == "h must have 2 dimensions, got 3"
    assert m.field(np.zeros((2, 2, 2))).shape == (2, 2, 2)      # no rank asked for


def test_field_wrong_rank_of_a_device_tensor_raises_the_text_passed_in():
    class Tensor(FakeDeviceTensor):
        def dim(self):
            return 2
    with pytest.raises(RuntimeError) as e:
        m.field(Tensor(), 1, "ref")
    assert str(e.value) == "ref must have 1 dimensions"
    with pytest.raises(RuntimeError) as e:
        m.field(Tensor(), 1, "ref", dev_message="ref must have 1 dimension")
    assert str(e.value) == "ref must have 1 dimension"


# ---- _wants_f64 -----------------------------------------------------------------------------------------------------------
def test_wants_f64_only_for_large_float64_arrays():
    big64, big32 = np.zeros((1024, 1024)), np.zeros((1024, 1024), np.float32)
    below = np.zeros((1 << 20) - 1)
    small32, small64 = np.zeros(5, np.float32), np.zeros(5)
    assert not m._wants_f64(below) and not m._wants_f64(small64) and not m._wants_f64()
    assert not m._wants_f64(big32) and not m._wants_f64(big32, small64)
    assert m._wants_f64(big64) and m._wants_f64(np.zeros(1 << 20))
    assert m._wants_f64(big64, small32) and m._wants_f64(small32, big64, None, [1.0, 2.0], 3.0)      # small companions do not count
    assert not m._wants_f64(big64, big32) and not m._wants_f64([[0.0]])                   # every large array must be float64
    import gridpp_amd
    assert gridpp_amd._wants_f64 is m._wants_f64


# ---- flags ----------------------------------------------------------------------------------------------------------------
def test_flags_of_host_fields():
    a, b = np.zeros(3, np.float32), np.zeros((2, 2), np.float32)
    assert m.flags(False, a) == _capi.MEM_HOST and m.flags(False, a, None, b) == _capi.MEM_HOST and m.flags(False) == _capi.MEM_HOST
    assert m.flags(True, a, b) == _capi.MEM_HOST | _capi.HOST_F64
    assert _capi.MEM_HOST | _capi.HOST_F64 != _capi.MEM_HOST


def test_flags_refuses_mixed_memory_before_any_synchronise(monkeypatch):
    def no_sync(mem):
        raise AssertionError("synchronised before the fields were checked")
    monkeypatch.setattr(m, "_sync_if_dev", no_sync)
    for f64 in (False, True):
        for fields in ((np.zeros(3, np.float32), FakeDeviceTensor()), (FakeDeviceTensor(), None, np.zeros(3, np.float32))):
            with pytest.raises(ValueError) as e:
                m.flags(f64, *fields)
            assert str(e.value) == "either all field arguments are torch CUDA tensors or none is"


def test_run_allocates_where_like_lives_and_appends_out_and_mem():
    seen = []

    def entry(a, b, out, mem):
        seen.append((a, b, mem))
        np.ctypeslib.as_array((_capi.C.c_float * 6).from_address(out.value)).fill(7)
        return _capi.GPP_OK
    out = m.run(entry, 1, "x", out_shape=(2, 3), like=np.zeros(1, np.float32), mem=_capi.MEM_HOST | _capi.HOST_F64)
    assert seen == [(1, "x", _capi.MEM_HOST | _capi.HOST_F64)]
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (2, 3) and (out == 7).all()
