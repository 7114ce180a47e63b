"""Tile lists of the grid kernel's primary batches: an item
builds the list of the small spheres its tile's camera rays can meet, and its
batches test that list in place of the grid walk.  The list only ever adds
spheres, so every image must still equal the oracle's fast mode bit for bit,
with the world.hit count equal: tiles with a list, with an empty list, over
the cap (the walk beside listed tiles), partial tiles, strips whose rows lie
far apart, depth limits at the batch's own segment, wide apertures, a camera
among the spheres, the general (several y layers) grid, an exact tie between
coincident spheres, items under the sample count that builds a list, the cost
probe, and the global-memory grid kinds, which keep the walk.

Items need kTileListMinSpp = 4 samples to build a list: 16 spp in the
automatic four items per tile is the least that does."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd as rt
import oracle_py as O
from test_grid_strides import stacked_scene
from test_tile_list import aperture2_camera, inside_camera, tile_lists

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_LIB = os.path.join(REPO, "a_dive_into_ray_tracing_amd", "lib", "librtmi_stats.so")
SEED = 1984


def o_cam(cam):
    c = O.OrCamera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(c))
    return c


def o_scene(world):
    return O.Scene(world.center_radius, world.mat_kind, world.mat_params)


_ORACLE = {}


def oracle(world, key, cam, W, H, S, D, rows=(0, 1, None)):
    """(image, world.hit count) of the oracle's fast mode, computed once per case."""
    k = (key, W, H, S, D, rows)
    if k not in _ORACLE:
        sc, oc = o_scene(world), o_cam(cam)
        _ORACLE[k] = (O.fast_render(sc, oc, W, H, S, D, SEED, *rows), O.fast_segments(sc, oc, W, H, S, D, SEED, *rows))
    return _ORACLE[k]


def check(r, world, key, cam, W, H, S, D, walks=(2,)):
    got = r.render(cam, W, H, S, D, SEED)
    segs = r.last_segments()
    sch = r.last_schedule()
    assert sch["bvh"] in walks and sch["persistent"] == 0, sch
    want, want_segs = oracle(world, key, cam, W, H, S, D)
    assert np.array_equal(got, want), f"max |d| {np.abs(got - want).max()}"
    assert segs == want_segs, (segs, want_segs)
    return sch


def grid_renderer_of(world):
    r = rt.Renderer(world, 0)
    r.set_kernel("grid")
    r.set_accel("grid")
    return r


@pytest.fixture(scope="module")
def final_world():
    return rt.random_scene()


@pytest.fixture(scope="module")
def grid_renderer(final_world):
    r = grid_renderer_of(final_world)
    yield r
    r.close()


@pytest.mark.parametrize("W,H", [(48, 32), (45, 29), (16, 96)])
def test_final_scene(W, H, final_world, grid_renderer):
    """48 x 32: tiles with a list beside tiles over the cap; 45 x 29: partial
    tiles; 16 x 96: the top tiles' lists are empty.  (The premises are checked
    on the host's lists.)"""
    cam = rt.final_camera(W / H)
    _, cnt, _ = tile_lists(final_world, cam, W, H)
    assert (cnt > 0).any()
    if (W, H) == (16, 96):
        assert (cnt[-4:] == 0).all(), cnt
    else:
        assert (cnt < 0).any(), cnt
    check(grid_renderer, final_world, "final", cam, W, H, 16, 50)


def test_strip_of_rows_far_apart(final_world, grid_renderer):
    """Rows 3, 11, ..., 59 of 96 x 64 in 16 x 4 tiles: a tile's rows lie 8 apart."""
    import torch

    W, H, S, row0, step, nrows = 96, 64, 16, 3, 8, 8
    cam = rt.final_camera(W / H)
    _, cnt, _ = tile_lists(final_world, cam, W, H, row0, step, nrows, tile_w=16)
    assert (cnt > 0).any() and (cnt < 0).any()
    want, want_segs = oracle(final_world, "final", cam, W, H, S, 50, rows=(row0, step, nrows))
    strip = torch.full((nrows, W, 3), -1.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    grid_renderer.set_tuning(16, 0)
    try:
        grid_renderer.render_rows(cam, W, H, S, 50, SEED, row0, step, nrows, strip.data_ptr(), st.cuda_stream)
        st.synchronize()
    finally:
        grid_renderer.set_tuning(0, 0)
    assert grid_renderer.last_schedule()["tile_w"] == 16
    assert np.array_equal(strip.cpu().numpy(), want)
    assert grid_renderer.last_segments() == want_segs


@pytest.mark.parametrize("depth", [1, 2])
def test_depth_limits(depth, final_world, grid_renderer):
    """max_depth 1: every path ends in its batch; 2: in its first pass after it."""
    check(grid_renderer, final_world, "final", rt.final_camera(48 / 32), 48, 32, 16, depth)


@pytest.mark.parametrize("S", [1, 3])
def test_items_under_the_list_threshold(S, final_world, grid_renderer):
    """Items of fewer than 4 samples build no list."""
    check(grid_renderer, final_world, "final", rt.final_camera(48 / 32), 48, 32, S, 50)


def test_one_item_per_tile(final_world, grid_renderer):
    """All 16 samples of a tile in one item (one list per tile, four batches)."""
    grid_renderer.set_schedule(1000, -1, 0)
    try:
        sch = check(grid_renderer, final_world, "final", rt.final_camera(48 / 32), 48, 32, 16, 50)
    finally:
        grid_renderer.set_schedule(0, -1, 0)
    assert sch["items_per_tile"] == 1, sch


@pytest.mark.parametrize("case", ["learn", "learn_aperture2", "final_aperture2", "inside"])
def test_cameras(case, final_world):
    """The learn scene (aperture 0.5), a lens disk of radius 1 (the final
    scene's tiles are all over the cap, the learn scene's few spheres fit),
    and a camera inside the layer of small spheres."""
    W, H = 48, 32
    world = final_world if case in ("final_aperture2", "inside") else rt.learn_scene()
    cam = {"learn": rt.learn_camera, "learn_aperture2": aperture2_camera, "final_aperture2": aperture2_camera,
           "inside": inside_camera}[case](W / H)
    r = grid_renderer_of(world)
    try:
        check(r, world, case, cam, W, H, 16, 50)
    finally:
        r.close()


def test_stacked_scene_general_walk():
    """A grid of several y layers: render_kernel<.., 2>."""
    world = stacked_scene()
    cam = rt.camera((13, 2, 3), (0, 0, 0), (0, 1, 0), 40.0, 48 / 32, 0.1, 10.0)
    _, cnt, _ = tile_lists(world, cam, 48, 32)
    assert (cnt > 0).any()
    r = grid_renderer_of(world)
    try:
        assert r.grid_info()[0][1] > 1
        check(r, world, "stacked", cam, 48, 32, 16, 50)
    finally:
        r.close()


def test_coincident_spheres_tie_goes_to_the_later_index():
    """Two spheres with the same centre and radius and different colours, in
    view: every root is an exact tie, which the later scene index wins
    (hittable_list.h:25-31) — the oracle's in-order loop does that by itself."""
    g = np.random.default_rng(3)
    n = 24
    c = np.column_stack([g.uniform(-4, 4, n), np.full(n, 0.2), g.uniform(-4, 4, n)])
    cr = np.vstack([[0, -1000, 0, 1000], np.column_stack([c, np.full(n, 0.2)]), [4, 0.7, 1, 0.7], [4, 0.7, 1, 0.7]])
    kinds = np.zeros(len(cr), np.int32)
    params = np.full((len(cr), 4), 0.5)
    params[-2, :3] = (0.9, 0.1, 0.1)
    params[-1, :3] = (0.1, 0.1, 0.9)
    world = rt.World(cr, kinds, params)
    W, H = 48, 32
    cam = rt.final_camera(W / H)
    idx, cnt, _ = tile_lists(world, cam, W, H)
    both = [t for t in range(len(cnt)) if {len(cr) - 2, len(cr) - 1} <= set(idx[t, :max(cnt[t], 0)])]
    assert both, cnt  # the pair is in some tile's list
    r = grid_renderer_of(world)
    try:
        check(r, world, "tie", cam, W, H, 16, 50)
    finally:
        r.close()
    want = oracle(world, "tie", cam, W, H, 16, 50)[0]
    assert (want[..., 2] > 2 * want[..., 0]).any()  # the blue one shows


def test_cost_probe_one_shot(final_world):
    """A first render with ordering `cost`: the 1-spp probe (no lists), then
    the render (lists)."""
    W, H, S = 64, 40, 16
    r = grid_renderer_of(final_world)
    try:
        r.set_ordering("cost")
        check(r, final_world, "final", rt.final_camera(W / H), W, H, S, 50)
    finally:
        r.close()


_CHILD = """
import ctypes as C, json, sys
sys.path[:0] = [{repo!r}, {tests!r}]
import a_dive_into_ray_tracing_amd as rt
import test_gpu_tile_list as t
world = rt.random_scene()
r = t.grid_renderer_of(world)
t.check(r, world, "final", rt.final_camera(48 / 32), 48, 32, 16, 50, walks=({walk},))
v = (C.c_uint64 * 8)()
if {stats}:
    L = rt.load()
    L.rt_ctx_debug_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    assert L.rt_ctx_debug_counters(r._h, v) == 0
r.close()
print("child ok", json.dumps(dict(cells=v[5], sphere_tests=v[6])))
"""


def run_child(env, walk=2, stats=False):
    code = _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), walk=walk, stats=stats)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stdout + p.stderr
    return json.loads(p.stdout.split("child ok", 1)[1])


@pytest.mark.parametrize("cap", [0, 1, 2, 32])
def test_list_cap_knob(cap):
    """RTMI_TILE_LIST_MAX in a fresh process: 0 no lists, 1 and 2 the walk
    beside the few tiles whose lists are that short, 32 the default."""
    run_child({"RTMI_TILE_LIST_MAX": str(cap)})


def test_grid_in_global_memory_keeps_the_walk():
    """RTMI_GRID_GLOBAL=1: kinds 4 / 5 build no list."""
    run_child({"RTMI_GRID_GLOBAL": "1"}, walk=4)


@pytest.mark.skipif(not os.path.exists(STATS_LIB), reason="needs the work-counting build")
def test_lists_replace_cell_visits():
    """The work-counting build: with lists the launch visits fewer cells (a
    listed batch visits none) and equals the oracle either way."""
    with_lists = run_child({"RTMI_LIBRARY": STATS_LIB}, stats=True)
    without = run_child({"RTMI_LIBRARY": STATS_LIB, "RTMI_TILE_LIST_MAX": "0"}, stats=True)
    assert 0 < with_lists["cells"] < without["cells"], (with_lists, without)
