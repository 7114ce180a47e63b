"""The big spheres in the tile lists on the GPU: a tile's list
names the big spheres its camera rays can meet as well, and its primary batches
test the list alone — no big group.  The list only ever adds spheres, so every
image must still equal the oracle's fast mode bit for bit, with the world.hit
count equal: tiles of pure sky (nothing to test), tiles that meet one big
sphere and nothing else, an exact tie between two coincident big spheres (the
later scene index wins, here through the slot index table), 1 to 8 big spheres
(the padded slots of the groups of four are never named), 9 (no big spheres in
the lists: the group as before), a camera inside a big glass sphere, depth
limits at the batch's own segment, and RTMI_TILE_BIG=0.

48 x 32 at 16 spp in the automatic four items a tile: the least that builds lists."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd as rt
from test_gpu_tile_list import REPO, STATS_LIB, check, grid_renderer_of
from test_tile_big import big_spheres, many_big_scene, tile_big
from test_tile_list import tile_lists

pytestmark = pytest.mark.gpu

W, H, S = 48, 32, 16


def sky_scene():
    """The ground, a glass sphere in the air, a diffuse and a metal one on the
    ground, 24 small spheres around them."""
    g = np.random.default_rng(21)
    n = 24
    w = rt.World()
    w.add(rt.sphere((0, -1000, 0), 1000, rt.lambertian((0.5, 0.5, 0.5))))
    for i in range(n):
        mat = [rt.lambertian(g.uniform(0.1, 0.9, 3)), rt.metal(g.uniform(0.5, 1, 3), g.uniform(0, 0.5)), rt.dielectric(1.5)][i % 3]
        w.add(rt.sphere((g.uniform(-4, 4), 0.2, g.uniform(-4, 4)), 0.2, mat))
        if i == 11:  # (the big ones among the small ones in scene order)
            w.add(rt.sphere((0, 6.75, 0), 1.0, rt.dielectric(1.5)))
            w.add(rt.sphere((-4, 1, 0), 1.0, rt.lambertian((0.4, 0.2, 0.1))))
    w.add(rt.sphere((4, 1, 0), 1.0, rt.metal((0.7, 0.6, 0.5), 0.0)))
    return w


def sky_camera():
    """From far and high, so that tiles of 8 x 8 pixels are narrow bundles: the
    top tile row lies above the horizon of the grown ground, the glass sphere
    in its middle."""
    return rt.camera((40, 8, 9), (0, 3, 0), (0, 1, 0), 14.0, W / H, 0.1, 41.0)


@pytest.fixture(scope="module")
def sky_world():
    return sky_scene()


@pytest.fixture(scope="module")
def sky_renderer(sky_world):
    r = grid_renderer_of(sky_world)
    yield r
    r.close()


def test_sky_tiles_and_tiles_of_one_big_sphere(sky_world, sky_renderer):
    cam = sky_camera()
    big, _ = big_spheres(sky_world)
    assert len(big) == 4
    idx, nb, _ = tile_big(sky_world, cam, W, H)
    _, ns, _ = tile_lists(sky_world, cam, W, H)
    assert (ns >= 0).all()
    assert ((nb == 0) & (ns == 0)).any(), (nb, ns)  # pure sky
    assert ((nb == 1) & (ns == 0) & (idx[:, 0] != big[0])).any(), (idx, ns)  # the glass sphere alone
    assert ((nb > 0) & (ns > 0)).any()
    check(sky_renderer, sky_world, "sky", cam, W, H, S, 50, walks=(2, 3))


@pytest.mark.parametrize("depth", [1, 2])
def test_depth_limits(depth, sky_world, sky_renderer):
    """max_depth 1: every path ends in its batch; 2: in its first pass after it."""
    check(sky_renderer, sky_world, "sky", sky_camera(), W, H, S, depth, walks=(2, 3))


def test_coincident_big_spheres_tie_goes_to_the_later_index():
    """Two big spheres with the same centre and radius and different colours:
    every root is an exact tie between two big slots."""
    g = np.random.default_rng(3)
    n = 24
    c = np.column_stack([g.uniform(-4, 4, n), np.full(n, 0.2), g.uniform(-4, 4, n)])
    cr = np.vstack([[0, -1000, 0, 1000], [2, 1, 1, 1], np.column_stack([c, np.full(n, 0.2)]), [2, 1, 1, 1]])
    kinds = np.zeros(len(cr), np.int32)
    params = np.full((len(cr), 4), 0.5)
    params[1, :3] = (0.9, 0.1, 0.1)
    params[-1, :3] = (0.1, 0.1, 0.9)
    world = rt.World(cr, kinds, params)
    cam = rt.final_camera(W / H)
    idx, nb, _ = tile_big(world, cam, W, H)
    assert any({1, len(cr) - 1} <= set(idx[t, :nb[t]]) for t in range(len(nb)))
    r = grid_renderer_of(world)
    try:
        check(r, world, "bigtie", cam, W, H, S, 50, walks=(2, 3))
    finally:
        r.close()
    from test_gpu_tile_list import oracle

    want = oracle(world, "bigtie", cam, W, H, S, 50)[0]
    assert (want[..., 2] > 2 * want[..., 0]).any()  # the blue one shows


@pytest.mark.parametrize("nbig", [1, 2, 3, 5, 8, 9])
def test_big_sphere_counts(nbig):
    """Groups of four with 3, 2, 1, 3 and 0 padded slots; 9: no big spheres in the lists."""
    world = many_big_scene(nbig)
    cam = rt.final_camera(W / H)
    assert len(big_spheres(world)[0]) == nbig
    _, nb, _ = tile_big(world, cam, W, H)
    assert (nb == -1).all() if nbig > 8 else (nb > 0).any()
    _, ns, _ = tile_lists(world, cam, W, H)
    assert (ns >= 0).any()
    r = grid_renderer_of(world)
    try:
        assert r.accel_info()[0] == nbig
        check(r, world, f"big{nbig}", cam, W, H, S, 50, walks=(2, 3))
    finally:
        r.close()


def test_camera_inside_a_big_glass_sphere():
    world = rt.random_scene()
    cam = rt.camera((0.2, 1.1, 0.3), (4, 1, 0), (0, 1, 0), 50.0, W / H, 0.05, 3.0)
    _, ns, _ = tile_lists(world, cam, W, H)
    assert (ns >= 0).any()
    r = grid_renderer_of(world)
    try:
        check(r, world, "inside_glass", cam, W, H, S, 50, walks=(2, 3))
    finally:
        r.close()


_CHILD = """
import ctypes as C, json, sys
sys.path[:0] = [{repo!r}, {tests!r}]
import a_dive_into_ray_tracing_amd as rt
import test_gpu_tile_big as t
world = t.sky_scene()
r = t.grid_renderer_of(world)
t.check(r, world, "sky", t.sky_camera(), t.W, t.H, t.S, 50, walks=(2, 3))
v = (C.c_uint64 * 8)()
if {stats}:
    L = rt.load()
    L.rt_ctx_debug_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    assert L.rt_ctx_debug_counters(r._h, v) == 0
r.close()
print("child ok", json.dumps(dict(cells=v[5], sphere_tests=v[6])))
"""


def run_child(env, stats=False):
    code = _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), stats=stats)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stdout + p.stderr
    return json.loads(p.stdout.split("child ok", 1)[1])


@pytest.mark.parametrize("knob", ["0", "1", None])
def test_knob(knob):
    """RTMI_TILE_BIG in a fresh process: 0 the big group in every batch, 1 and unset the default."""
    run_child({} if knob is None else {"RTMI_TILE_BIG": knob})


def test_the_lists_carry_the_big_tests():
    """The work-counting build: the list loop's sphere tests count the big
    spheres it tests, so there are more of them than with RTMI_TILE_BIG=0
    (where the uncounted big group tests them), over the same cell visits."""
    assert os.path.exists(STATS_LIB)
    on = run_child({"RTMI_LIBRARY": STATS_LIB}, stats=True)
    off = run_child({"RTMI_LIBRARY": STATS_LIB, "RTMI_TILE_BIG": "0"}, stats=True)
    assert on["cells"] == off["cells"] > 0 and on["sphere_tests"] > off["sphere_tests"], (on, off)
