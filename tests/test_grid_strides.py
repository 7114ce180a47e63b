"""The grid descriptor's cell-start strides (host only, no device): the walk
forms a cell's address as cells + 4 cx + row_bytes cy + layer_bytes cz with
24-bit multiplies, so the strides must be 4 n0 and 4 n0 n1, the cell
coordinates below 2^16 and the strides below 2^24; a grid that breaks the
bound is refused where it is built."""
import ctypes as C

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd as rt


def lib():
    L = rt.load()
    L.rt_debug_grid_strides.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    L.rt_debug_grid_strides.restype = C.c_int
    L.rt_debug_grid_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    L.rt_debug_grid_layout.restype = C.c_int
    return L


def strides(n3):
    out = (C.c_uint32 * 2)()
    rc = lib().rt_debug_grid_strides((C.c_int32 * 3)(*n3), out)
    return rc, tuple(out)


def stacked_scene():
    g = np.random.default_rng(8)
    n = 300
    c = g.uniform(-6, 6, (n, 3))
    c[:, 1] = g.uniform(-0.5, 7, n)
    r = np.exp(g.uniform(np.log(0.02), np.log(0.9), n))
    cr = np.vstack([[0, -1000, 0, 1000], np.column_stack([c, r])])
    kinds = np.zeros(n + 1, np.int32)
    params = np.full((n + 1, 4), 0.5)
    return rt.World(cr, kinds, params)


@pytest.mark.parametrize("name", ["final", "learn", "stacked"])
def test_strides_of_the_fixture_scenes(name):
    world = {"final": rt.random_scene, "learn": rt.learn_scene, "stacked": stacked_scene}[name]()
    sc = world.c_struct()
    dims, st, box = (C.c_int32 * 3)(), (C.c_uint32 * 2)(), (C.c_float * 6)()
    rc = lib().rt_debug_grid_layout(C.byref(sc), dims, st, box)
    assert rc == 0, rt.load().rt_last_error()
    n0, n1, n2 = dims
    assert min(n0, n1, n2) >= 1 and n0 * n1 * n2 <= 16384
    if name == "final":
        assert n1 == 1, tuple(dims)  # the one-layer walk's scene
    if name == "stacked":
        assert n1 > 1, tuple(dims)
    assert tuple(st) == (4 * n0, 4 * n0 * n1)
    assert all(h > 0 for h in box[3:])


@pytest.mark.parametrize("n3", [(1, 1, 1), (20, 1, 20), (7, 5, 3), (128, 128, 1), (65535, 1, 1), (1024, 4095, 1), (2, 3, 65535)])
def test_strides_within_the_bound(n3):
    rc, st = strides(n3)
    assert rc == 0
    assert st == (4 * n3[0], 4 * n3[0] * n3[1])
    assert st[1] < 1 << 24 and max(n3) < 1 << 16


@pytest.mark.parametrize("n3", [(65536, 1, 1), (1, 65536, 1), (1, 1, 65536), (1024, 4096, 1), (4096, 1024, 2), (0, 1, 1),
                                (4, -1, 4)])
def test_grid_over_the_24_bit_bound_is_refused(n3):
    rc, _ = strides(n3)
    assert rc != 0
    assert b"24-bit" in rt.load().rt_last_error()
