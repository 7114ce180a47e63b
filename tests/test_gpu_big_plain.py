"""The big-sphere group in plain FMAs (hit_big) on the GPU.
The group forms hb and disc of its four slots by sphere_test's chains with the
sphere's values as scalar operands; every bit must be what the packed form
gave, so:

1. the closest hit of constructed rays (index and t) equals the brute-force
   loop's, which stays packed, for 1 to 9 big spheres (groups with 3, 2, 1, 0,
   3, 0 and 3 padded slots) and for two coincident big spheres, through all
   three instantiations of hit_big (the grid's keys, the BVH's indices, the
   grid walked in global memory);
2. images equal the oracle's fast mode bit for bit with the group forced into
   every batch (RTMI_TILE_BIG=0) and at the default, and the BVH's image
   equals brute force's;
3. the work-counting build renders the product's image and counts the group's
   resolutions.

100 000 rays and 48 x 32 x 16 spp: each case takes about a second."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd as rt
from test_gpu_tile_list import REPO, SEED, STATS_LIB, check, grid_renderer_of
from test_tile_big import big_spheres, many_big_scene

pytestmark = pytest.mark.gpu

W, H, S = 48, 32, 16
NRAYS = 100_000
SCENES = [1, 2, 3, 4, 5, 8, 9, "tie"]


def tie_scene():
    """The ground and two coincident big spheres (scene indices 1 and 26)
    among 24 small ones: every root on them is an exact tie between two big slots."""
    g = np.random.default_rng(3)
    n = 24
    c = np.column_stack([g.uniform(-4, 4, n), np.full(n, 0.2), g.uniform(-4, 4, n)])
    cr = np.vstack([[0, -1000, 0, 1000], [2, 1, 1, 1], np.column_stack([c, np.full(n, 0.2)]), [2, 1, 1, 1]])
    params = np.full((len(cr), 4), 0.5)
    params[1, :3] = (0.9, 0.1, 0.1)
    params[-1, :3] = (0.1, 0.1, 0.9)
    return rt.World(cr, np.zeros(len(cr), np.int32), params)


def scene_of(which):
    return tie_scene() if which == "tie" else many_big_scene(which)


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def big_rays(world, n=NRAYS, seed=17):
    """float32 rays {o, d} [n, 6] aimed at the big spheres.

    First half: origins on a big sphere's surface at relative offsets
    {+1e-3, +1e-4, -1e-4, +1e-6, 0} (the ground's near its top, where the scene
    is), a third of them with tangent directions (exactly perpendicular to the
    radius in float64: disc rounds to either sign), a third straight away from
    the sphere, a third anywhere.  Then a fifth inside a big sphere (below the
    ground's top, or within 0.9 radii of a centre), a tenth high above the
    scene looking up (away from every big sphere: both roots negative, a
    miss), the rest from the field.  3 % of the direction components are
    exactly +0.0 or -0.0."""
    g = np.random.default_rng(seed)
    big, cr = big_spheres(world)
    h = n // 2
    k = big[g.integers(0, len(big), h)]
    c, rad = cr[k, :3], np.abs(cr[k, 3])
    u = unit(g.normal(size=(h, 3)))
    top = unit(np.column_stack([g.uniform(-8, 8, h) / 1000, np.ones(h), g.uniform(-8, 8, h) / 1000]))
    u = np.where((rad > 100)[:, None], top, u)
    o = np.empty((n, 3))
    o[:h] = c + u * (rad * (1 + g.choice([1e-3, 1e-4, -1e-4, 1e-6, 0.0], h)))[:, None]
    d = g.normal(size=(n, 3)) * g.choice([0.3, 1.0, 3.0], n)[:, None]
    third = h // 3
    tang = np.cross(u[:third], g.normal(size=(third, 3)))
    d[:third] = unit(tang) * g.choice([0.3, 1.0, 3.0], third)[:, None]
    d[third:2 * third] = u[third:2 * third] * g.choice([0.3, 1.0, 3.0], third)[:, None]
    # inside a big sphere
    m = n // 5
    ki = big[g.integers(0, len(big), m)]
    ci, ri = cr[ki, :3], np.abs(cr[ki, 3])
    inside = ci + unit(g.normal(size=(m, 3))) * (ri * g.uniform(0, 0.9, m))[:, None]
    under = np.column_stack([g.uniform(-8, 8, m), -g.uniform(0.01, 5, m), g.uniform(-8, 8, m)])
    o[h:h + m] = np.where((ri > 100)[:, None], under, inside)
    # above everything, looking up
    a = n // 10
    o[h + m:h + m + a] = np.column_stack([g.uniform(-8, 8, a), g.uniform(3, 6, a), g.uniform(-8, 8, a)])
    d[h + m:h + m + a, 1] = np.abs(d[h + m:h + m + a, 1]) + 0.01
    # the field
    rest = n - (h + m + a)
    o[h + m + a:] = np.column_stack([g.uniform(-8, 8, rest), g.uniform(-0.1, 3, rest), g.uniform(-8, 8, rest)])
    z = g.random((n, 3)) < 0.03
    z[h + m:h + m + a, 1] = False  # (these keep looking up)
    d[z] = np.where(g.random(int(z.sum())) < 0.5, 0.0, -0.0)
    d[np.all(d == 0, axis=1)] = [0, -1, 0]  # no zero directions (not a ray)
    return np.ascontiguousarray(np.column_stack([o, d]).astype(np.float32))


def f64_shares(world, rays):
    """(share of rays whose closest hit in [0.001, inf) is a big sphere, share that
    miss everything) in float64 from o - c: what the recipe gives before any GPU run."""
    big, cr = big_spheres(world)
    o, d = rays[:, None, :3].astype(np.float64), rays[:, None, 3:].astype(np.float64)
    oc = o - cr[None, :, :3]
    a = (d * d).sum(2)
    hb = (oc * d).sum(2)
    cc = (oc * oc).sum(2) - cr[None, :, 3] ** 2
    disc = hb * hb - a * cc
    sq = np.sqrt(np.maximum(disc, 0))
    t1, t2 = (-hb - sq) / a, (-hb + sq) / a
    t = np.where(t1 >= 1e-3, t1, np.where(t2 >= 1e-3, t2, np.inf))
    t[disc < 0] = np.inf
    first = t.argmin(1)
    hit = np.isfinite(t.min(1))
    return float((hit & np.isin(first, big)).mean()), float((~hit).mean())


_RAYS = {}


def rays_of(which):
    if which not in _RAYS:
        world = scene_of(which)
        rays = big_rays(world)
        _RAYS[which] = (world, rays, f64_shares(world, rays))
    return _RAYS[which]


def debug_hits(r, rays):
    L = rt.load()
    L.rt_ctx_debug_hits.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    n = len(rays)
    idx, t = np.zeros(2 * n, np.int32), np.zeros(2 * n, np.float32)
    rc = L.rt_ctx_debug_hits(r._h, rays.ctypes.data_as(C.POINTER(C.c_float)), n, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                             t.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0, L.rt_last_error()
    return idx.reshape(n, 2), t.reshape(n, 2)


@pytest.mark.parametrize("accel", ["grid", "bvh", "grid_global"])
@pytest.mark.parametrize("which", SCENES)
def test_closest_hit_equals_brute_force(which, accel, monkeypatch):
    world, rays, (big_share, miss_share) = rays_of(which)
    big, _ = big_spheres(world)
    assert len(big) == (3 if which == "tie" else which)
    # the recipe, in float64, before the GPU sees it
    print(f"{which} {accel}: float64 big {big_share:.4f} miss {miss_share:.4f}")
    assert big_share >= 0.25 and miss_share >= 0.01, (big_share, miss_share)
    if accel == "grid_global":
        monkeypatch.setenv("RTMI_GRID_GLOBAL", "1")
    r = rt.Renderer(world, 0)
    try:
        r.set_accel(accel.split("_")[0])
        assert r.accel_info()[0] == len(big)
        idx, t = debug_hits(r, rays)
        # the instantiation that ran: a one-pixel render's kind (1 BVH, 2 / 3 grid, 4 / 5 the grid in global memory)
        r.render(rt.final_camera(1.0), 8, 8, 1, 2, SEED)
        assert r.last_schedule()["bvh"] in {"grid": (2, 3), "bvh": (1,), "grid_global": (4, 5)}[accel], r.last_schedule()
    finally:
        r.close()
    got_big, got_miss = float(np.isin(idx[:, 0], big).mean()), float((idx[:, 0] < 0).mean())
    print(f"{which} {accel}: brute force big {got_big:.4f} miss {got_miss:.4f}")
    assert got_big >= 0.25 and got_miss >= 0.01, (got_big, got_miss)
    if which == "tie":  # the later of the coincident pair wins every tie
        assert (idx[:, 0] == len(world) - 1).any() and not (idx[:, 0] == 1).any()
    bad = np.flatnonzero((idx[:, 0] != idx[:, 1]) | (t[:, 0] != t[:, 1]))
    assert bad.size == 0, (bad.size, rays[bad[:4]], idx[bad[:4]], t[bad[:4]])


_CHILD = """
import ctypes as C, json, sys
import numpy as np
sys.path[:0] = [{repo!r}, {tests!r}]
import a_dive_into_ray_tracing_amd as rt
import test_gpu_big_plain as t
v = (C.c_uint64 * 8)()
for which in {scenes!r}:
    world = t.scene_of(which)
    r = t.grid_renderer_of(world)
    t.check(r, world, f"plain{{which}}", rt.final_camera(t.W / t.H), t.W, t.H, t.S, 50, walks=(2, 3))
    if {stats}:
        L = rt.load()
        L.rt_ctx_debug_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        assert L.rt_ctx_debug_counters(r._h, v) == 0
        np.save({image!r}, r.render(rt.final_camera(t.W / t.H), t.W, t.H, t.S, 50, t.SEED))
    r.close()
print("child ok", json.dumps(dict(root_resolutions_wave=v[4])))
"""


def run_child(env, scenes, stats=False, image=""):
    code = _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), scenes=scenes, stats=stats, image=image)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stdout + p.stderr
    return json.loads(p.stdout.split("child ok", 1)[1])


@pytest.mark.parametrize("knob", ["0", None])
def test_images_equal_the_oracle(knob):
    """Every scene against the oracle's fast mode (image and world.hit count)
    in a fresh process: RTMI_TILE_BIG=0 runs the group in every batch, the
    default leaves it to the secondary segments and the batches without a list."""
    run_child({} if knob is None else {"RTMI_TILE_BIG": knob}, SCENES)


def test_bvh_image_equals_brute_force():
    world = scene_of(5)
    cam = rt.final_camera(W / H)
    img = {}
    for accel in ("bvh", "none"):
        r = rt.Renderer(world, 0)
        try:
            r.set_accel(accel)
            img[accel] = r.render(cam, W, H, S, 50, SEED)
            assert r.last_schedule()["bvh"] == (1 if accel == "bvh" else 0), r.last_schedule()
        finally:
            r.close()
    assert np.array_equal(img["bvh"], img["none"])


def test_work_counting_build_renders_the_same_image(tmp_path):
    assert os.path.exists(STATS_LIB)
    world = scene_of(5)
    r = grid_renderer_of(world)
    try:
        want = r.render(rt.final_camera(W / H), W, H, S, 50, SEED)
    finally:
        r.close()
    image = str(tmp_path / "stats.npy")
    counts = run_child({"RTMI_LIBRARY": STATS_LIB}, [5], stats=True, image=image)
    assert np.load(image).tobytes() == want.tobytes()
    assert counts["root_resolutions_wave"] > 0, counts
