"""The structures rt_ctx_set_scene uploads, pinned byte for byte (host only, no
device): rt_debug_accel_digest returns one FNV-1a-64 per array the CPU
builders (csrc/rtmi_accel_build.cpp build_accel) give for a scene — the big
slots' index table, the BVH nodes, its leaf records and indices, the grid
descriptor's scalars, cells, refs, the tile table and the global-memory grid
image — and tests/golden/accel_digests.txt holds the values of the commit
before the builders moved into a host file of their own.  A change that only
moves or tidies builder code must leave every value as it is; a failure names
the array that moved.

A later pull request that MEANS to change a structure (a margin, the cell
density, the split rule, a table layout) regenerates the file from its own
build (python tests/test_accel_digest.py > tests/golden/accel_digests.txt) and
says so in its description."""
import ctypes as C
import os

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd as rt
from test_grid_strides import stacked_scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "accel_digests.txt")
ARRAYS = ["big_slots", "bvh_nodes", "bvh_leaves", "grid_desc", "grid_cells", "grid_refs", "tile_table", "grid_image"]


def nine_big_scene():
    """100 spheres of radius 0.1 and 9 of radius 10: more than kTileBigMax (8)
    big spheres, so the tile table has no big part."""
    g = np.random.default_rng(14)
    small = np.column_stack([g.uniform(-4, 4, (100, 3)), np.full(100, 0.1)])
    big = np.column_stack([g.uniform(-40, 40, (9, 3)), np.full(9, 10.0)])
    cr = np.vstack([big[:4], small, big[4:]])  # big spheres at both ends of the scene order
    return rt.World(cr, np.zeros(109, np.int32), np.full((109, 4), 0.5))


SCENES = {"final": rt.random_scene, "learn": rt.learn_scene, "stacked": stacked_scene, "nine_big": nine_big_scene}


def digests(world):
    L = rt.load()
    L.rt_debug_accel_digest.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.rt_debug_accel_digest.restype = C.c_int
    sc, out = world.c_struct(), (C.c_uint64 * 8)()
    rc = L.rt_debug_accel_digest(C.byref(sc), out)
    assert rc == 0, L.rt_last_error()
    return [f"{v:016x}" for v in out]


def golden():
    rows = [ln.split() for ln in open(GOLDEN) if ln.strip() and not ln.startswith("#")]
    return {r[0]: r[1:] for r in rows}


@pytest.mark.parametrize("name", list(SCENES))
def test_structures_are_byte_identical(name):
    want, got = golden()[name], digests(SCENES[name]())
    assert len(want) == len(ARRAYS)
    moved = [a for a, w, g in zip(ARRAYS, want, got) if w != g]
    assert not moved, f"{name}: {moved} differ from tests/golden/accel_digests.txt"


def test_nine_big_scene_has_no_big_table():
    """The fourth scene is what it is meant to be: every tile's big count is -1."""
    from test_tile_big import tile_big
    _, cnt, _ = tile_big(nine_big_scene(), rt.final_camera(48 / 32), 48, 32)
    assert (cnt == -1).all()


if __name__ == "__main__":
    print("# scene " + " ".join(ARRAYS) + "  (FNV-1a-64 of each array, rt_debug_accel_digest)")
    for name, make in SCENES.items():
        print(name, *digests(make()))
