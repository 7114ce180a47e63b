"""The range guards of the kernels' exact float sqrt and reciprocal
(rtmi_path.h: rsqrt_cr, rcp_cr's unsigned range test) and the two forms
that were measured and not built into the render path (rtmi_device.hip:
sqrt_cr_zero_or_big for the sampling roots, sqrt_cr's short form with no
guard), checked exhaustively on the GPU through rt_debug_math_guards; the
enumeration of the sampling roots' arguments is repeated on the CPU
(DESIGN.md §4.5)."""
import ctypes as C

import numpy as np
import pytest

from a_dive_into_ray_tracing_amd import _abi

RT_EINVAL = -1  # include/rtmi.h

B_2M96 = 0x0F800000  # bits(2^-96)
B_2M126 = 0x00800000  # bits(2^-126), the smallest normal
B_INF = 0x7F800000


def _guards():
    f = _abi.load().rt_debug_math_guards
    f.argtypes = [C.c_int32, C.POINTER(C.c_uint64)]
    f.restype = C.c_int
    return f


def _run(form):
    v = (C.c_uint64 * 4)()
    rc = _guards()(form, v)
    assert rc == 0, f"rt_debug_math_guards({form}) returned {rc}"
    bad, first, pair, compared = (int(x) for x in v)
    print(f"form {form}: compared {compared}, mismatches {bad}, first input {first:#x}, "
          f"got {pair & 0xFFFFFFFF:#010x}, want {pair >> 32:#010x}")
    return bad, first, pair, compared


@pytest.mark.parametrize("form", [-1, 5, 2**31 - 1])
def test_unknown_form_is_einval(form):
    """An unknown form is refused before the entry point looks for a GPU."""
    v = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert _guards()(form, v) == RT_EINVAL
    assert list(v) == [7, 7, 7, 7]
    assert _guards()(0, None) == RT_EINVAL


@pytest.mark.gpu
@pytest.mark.parametrize("form,compared", [(0, 2**32), (1, 2**32), (2, 1 + (B_INF - B_2M96)), (3, 2 * 2**24)],
                         ids=["rsqrt_cr", "rcp_cr", "sqrt_zero_or_big", "sampling_arguments"])
def test_guard_forms_exhaustive(form, compared):
    """rsqrt_cr == 1.0f / sqrtf(x) and rcp_cr == 1.0f / x on all 2^32 bit
    patterns; sqrt_cr_zero_or_big == sqrtf(x) on every pattern of
    {+0} U [2^-96, inf); the sampling roots' arguments, formed on the GPU
    for all 2^24 uniforms, lie in that domain and sqrt_cr_zero_or_big equals
    sqrt_cr on them.  Bit patterns compared, NaN equal to NaN."""
    bad, first, pair, n = _run(form)
    assert n == compared
    assert bad == 0, f"{bad} mismatches; first input {first:#x}: got {pair & 0xFFFFFFFF:#010x}, want {pair >> 32:#010x}"


@pytest.mark.gpu
def test_unguarded_sqrt_probe():
    """The probe of DESIGN.md §8 item 4: sqrt_cr's short form with no guard on
    the small normals [2^-126, 2^-96).  It reports its mismatches (they
    decide whether the guard could become a test of the result); it asserts
    only that the whole range was compared.  On the MI355X 1 796 212 of the
    251 658 240 inputs differ from sqrtf by one ulp, the first 0x00800941:
    the guard stays a range test of the input."""
    bad, first, pair, n = _run(4)
    assert n == B_2M96 - B_2M126
    assert 0 <= bad <= n


def test_sampling_arguments_enumerated():
    """For every uniform u = k 2^-24 the two arguments of the sampling roots,
    fma(-z, z, 1) with z = fma(-2, u, 1) and u itself, are +0 exactly once
    (at u = 0), otherwise at least 2^-22 - 2^-46 (the float below 2^-22:
    u = 2^-24 gives z = 1 - 2^-23 and 1 - z^2 = 2^-22 - 2^-46 exactly) and
    2^-24, never negative or non-finite: inside {+0} U [2^-96, inf).  z is exact in float (an odd
    multiple of 2^-23 at most, |z| <= 1); z * z is exact in float64, so
    the fma is the float64 value rounded once."""
    u = np.arange(2**24, dtype=np.float64) * 2.0**-24
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    z = 1.0 - 2.0 * u
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
    arg = (1.0 - z * z).astype(np.float32)
    for a, smallest in ((arg, 2.0**-22 - 2.0**-46), (u.astype(np.float32), 2.0**-24)):
        bits = a.view(np.uint32)
        assert np.count_nonzero(bits == 0) == 1 and bits[0] == 0  # +0 (not -0), once, at u = 0
        nz = a[1:]
        assert np.isfinite(nz).all() and nz.min() == np.float32(smallest) and nz.max() <= 1.0
        assert ((bits[1:] >= B_2M96) & (bits[1:] < B_INF)).all()
    assert arg.max() == 1.0 and u.max() < 1.0
