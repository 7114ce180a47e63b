"""Primary batches of the grid kernels: the pool refill
traces and shades its 64 camera rays as one pass, accumulates the paths that
end there and hands the survivors out after their first bounce.  The cases
are the places where that can go wrong and the one-ray-at-a-time pool could
not: batches in which every path dies, partial tiles and partial last pools,
depth limits at and just above the batch's own segment, every item shape of
the schedule, every grid walk, and the cost probe.  Every image is compared
bit for bit with the oracle's fast mode, and the GPU's world.hit count with
the oracle's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd as rt
import oracle_py as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1984


def o_cam(cam):
    c = O.OrCamera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(c))
    return c


def o_scene(world):
    return O.Scene(world.center_radius, world.mat_kind, world.mat_params)


@pytest.fixture(scope="module")
def final_world():
    return rt.random_scene()


@pytest.fixture(scope="module")
def grid_renderer(final_world):
    r = rt.Renderer(final_world, 0)
    r.set_kernel("grid")
    r.set_accel("grid")
    yield r
    r.close()


_ORACLE = {}


def oracle(world, key, cam, W, H, S, D):
    """(image, world.hit count) of the oracle's fast mode, computed once per case."""
    k = (key, W, H, S, D)
    if k not in _ORACLE:
        sc, oc = o_scene(world), o_cam(cam)
        _ORACLE[k] = (O.fast_render(sc, oc, W, H, S, D, SEED), O.fast_segments(sc, oc, W, H, S, D, SEED))
    return _ORACLE[k]


def check(r, world, key, cam, W, H, S, D, walks=(2,)):
    got = r.render(cam, W, H, S, D, SEED)
    segs = r.last_segments()
    sch = r.last_schedule()
    # render_kernel ran on the grid (2: staged in LDS, 4: walked in global memory)
    assert sch["bvh"] in walks and sch["persistent"] == 0, sch
    want, want_segs = oracle(world, key, cam, W, H, S, D)
    assert np.array_equal(got, want), f"max |d| {np.abs(got - want).max()}"
    assert segs == want_segs, (segs, want_segs)
    return sch


@pytest.mark.parametrize("S", [3, 16])
def test_rows_that_see_only_sky(S, final_world, grid_renderer):
    """The final camera's top rows see only sky (a tall 16 x 96 image in 16 x 4
    tiles: the top tile is all sky): whole batches die there, one after the
    other, and the item ends on a dead batch; the tiles on the horizon end on
    a live one.  (The premise is checked: the oracle counts one world.hit per
    sample in the top 4 rows.)"""
    W, H = 16, 96
    cam = rt.final_camera(W / H)
    top = O.fast_segments(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED, row0=H - 4, row_step=1, nrows=4)
    assert top == W * 4 * S
    grid_renderer.set_tuning(16, 0)
    try:
        sch = check(grid_renderer, final_world, "final", cam, W, H, S, 50)
    finally:
        grid_renderer.set_tuning(0, 0)
    assert sch["tile_w"] == 16, sch


@pytest.mark.parametrize("tile_w", [8, 16])
@pytest.mark.parametrize("W,H,S", [(29, 19, 5), (29, 19, 1), (45, 11, 7)])
def test_partial_tiles_and_partial_last_pool(W, H, S, tile_w, final_world, grid_renderer):
    """Widths that are no multiple of 8 or 16, heights that are no multiple of
    the tile's, and job counts that are no multiple of 64."""
    cam = rt.final_camera(W / H)
    grid_renderer.set_tuning(tile_w, 0)
    try:
        sch = check(grid_renderer, final_world, "final", cam, W, H, S, 50)
    finally:
        grid_renderer.set_tuning(0, 0)
    assert sch["tile_w"] == tile_w, sch


@pytest.mark.parametrize("depth", [1, 2, 8])
def test_depth_limits(depth, final_world, grid_renderer):
    """max_depth 1: nothing survives a batch (sky or black); 2: every adopted
    path ends in its first pass; 8: the cost probe's depth."""
    W, H, S = 40, 24, 6
    cam = rt.final_camera(W / H)
    check(grid_renderer, final_world, "final", cam, W, H, S, depth)


@pytest.mark.parametrize("shape", ["small_chunk", "one_item", "auto", "tail", "overlap"])
def test_item_shapes(shape, final_world, grid_renderer):
    """Several items per tile (chunks of 3 of 10 samples: a last chunk of 1),
    one item per tile, the automatic four items of a block that owns its
    tile, a tail phase of short items, and the overlapped launch mode."""
    W, H, S = 40, 24, 10
    cam = rt.final_camera(W / H)
    r = grid_renderer
    try:
        if shape == "small_chunk":
            r.set_schedule(3, -1, 0)
        elif shape == "one_item":
            r.set_schedule(1000, -1, 0)
        elif shape == "tail":
            r.set_schedule(0, 4, 1)
        elif shape == "overlap":
            r.set_overlap(True)
        sch = check(r, final_world, "final", cam, W, H, S, 50)
    finally:
        r.set_schedule(0, -1, 0)
        r.set_overlap(False)
    if shape == "small_chunk":
        assert sch["chunk"] == 3 and sch["items_per_tile"] == 4, sch
    elif shape == "one_item":
        assert sch["items_per_tile"] == 1, sch
    elif shape == "auto":
        assert sch["block_flush"] == 2, sch  # the block owns its tile
    elif shape == "tail":
        assert sch["tail_items_per_tile"] > 0, sch


def test_accumulator_path(final_world, monkeypatch):
    """RTMI_BLOCK_OWNS=0: the block's sums go through the int64 accumulator."""
    W, H, S = 40, 24, 10
    cam = rt.final_camera(W / H)
    monkeypatch.setenv("RTMI_BLOCK_OWNS", "0")
    r = rt.Renderer(final_world, 0)
    try:
        r.set_kernel("grid")
        r.set_accel("grid")
        sch = check(r, final_world, "final", cam, W, H, S, 50)
    finally:
        r.close()
    assert sch["block_flush"] == 1, sch


def random_world(seed):
    """300 spheres as tests/test_gpu_parity.py builds them: radii over three
    decades, hollow shells, a coincident pair, two big spheres."""
    g = np.random.default_rng(seed)
    n = 300
    c = g.uniform(-8, 8, (n, 3))
    c[:, 1] = g.uniform(-0.5, 3, n)
    r = np.exp(g.uniform(np.log(0.01), np.log(1.5), n))
    r[g.random(n) < 0.05] *= -1
    c[10] = c[11]
    r[10] = r[11] = 0.3
    kinds = g.integers(0, 3, n).astype(np.int32)
    params = np.column_stack([g.uniform(0.1, 0.9, (n, 3)), np.where(kinds == 2, 1.5, g.uniform(0, 0.5, n))])
    cr = np.vstack([[0, -1000, 0, 1000], [0, 1, 40, 30], np.column_stack([c, r])])
    kinds = np.concatenate([[0, 1], kinds]).astype(np.int32)
    params = np.vstack([[0.5, 0.5, 0.5, 0], [0.7, 0.6, 0.5, 0.1], params])
    return rt.World(cr, kinds, params)


def test_grid_with_several_y_layers():
    """A random scene whose grid has more than one y layer: the general walk."""
    world = random_world(2)
    cam = rt.camera((13, 2, 3), (0, 0, 0), (0, 1, 0), 40.0, 1.5, 0.1, 10.0)
    r = rt.Renderer(world, 0)
    try:
        r.set_kernel("grid")
        r.set_accel("grid")
        assert r.grid_info()[0][1] > 1
        check(r, world, "random2", cam, 72, 48, 6, 50, walks=(2, 4))
    finally:
        r.close()


_CHILD = """
import sys
sys.path[:0] = [{repo!r}, {tests!r}]
import numpy as np
import a_dive_into_ray_tracing_amd as rt
import test_gpu_primary_batch as t
world = rt.random_scene()
cam = rt.final_camera(40 / 24)
r = rt.Renderer(world, 0)
r.set_kernel("grid")
r.set_accel("grid")
t.check(r, world, "final", cam, 40, 24, 6, 50, walks=(4,))
r.close()
print("child ok")
"""


def test_grid_walked_in_global_memory():
    """RTMI_GRID_GLOBAL=1 in a fresh process: the one-layer walk in global memory."""
    env = dict(os.environ, RTMI_GRID_GLOBAL="1")
    code = _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stdout + p.stderr


def test_cost_ordering_equals_none(final_world):
    """A one-shot render with ordering `cost` (the probe at depth 8, then the
    render) equals the render with ordering `none`, and the oracle."""
    W, H, S = 64, 40, 12
    cam = rt.final_camera(W / H)
    r = rt.Renderer(final_world, 0)
    try:
        r.set_kernel("grid")
        r.set_accel("grid")
        r.set_ordering("none")
        plain = r.render(cam, W, H, S, 50, SEED)
        plain_segs = r.last_segments()
        r.set_ordering("cost")
        check(r, final_world, "final", cam, W, H, S, 50)
        assert np.array_equal(plain, oracle(final_world, "final", cam, W, H, S, 50)[0])
        assert plain_segs == oracle(final_world, "final", cam, W, H, S, 50)[1]
    finally:
        r.close()
