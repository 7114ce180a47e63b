"""rt_debug_exact_math refuses a `which` it does not know before it looks for
a GPU (the checks themselves: tests/test_gpu_parity.py)."""
import ctypes as C

import pytest

from a_dive_into_ray_tracing_amd import _abi

RT_EINVAL = -1  # include/rtmi.h


@pytest.mark.parametrize("which", [-1, 2, 2**31 - 1])
def test_which_out_of_range_is_einval(which):
    L = _abi.load()
    f = L.rt_debug_exact_math
    f.argtypes = [C.c_int32, C.POINTER(C.c_uint64)]
    f.restype = C.c_int
    v = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert f(which, v) == RT_EINVAL
    assert list(v) == [7, 7, 7, 7]


def test_null_out_is_einval():
    L = _abi.load()
    f = L.rt_debug_exact_math
    f.argtypes = [C.c_int32, C.POINTER(C.c_uint64)]
    f.restype = C.c_int
    assert f(0, None) == RT_EINVAL
