"""The per-segment prologue of the grid walk: safe_inv, the
box clip, the entry cell and its clamp, the per-axis t0 / dt / kmax, the cell
address by the descriptor's byte strides, and the batch pass's job decode.
Every case is grid == brute force bit for bit on the same device: images
whose tiles are full and partial at tile widths 8 and 16, a strip of every
third row, max_depth 1, on the final scene (the one-layer walk) and on a
scene stacked in y (the general walk), each in LDS and in global memory; and
constructed rays through rt_ctx_debug_hits that start beyond each face of the
grid box, inside it and exactly on cell faces, run along the axes with +0.0,
-0.0 and 1e-25 components, and enter at the last cell of each axis."""
import ctypes as C

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd as rt

pytestmark = pytest.mark.gpu

SEED = 1984
SIZES = [(37, 19), (100, 13)]


def stacked_world():
    """300 random spheres stacked in y (several cell layers), hollow shells, a
    coincident pair, the ground and one more big sphere."""
    g = np.random.default_rng(8)
    n = 300
    c = g.uniform(-6, 6, (n, 3))
    c[:, 1] = g.uniform(-0.5, 7, n)
    r = np.exp(g.uniform(np.log(0.02), np.log(0.9), n))
    r[g.random(n) < 0.05] *= -1
    c[10] = c[11]
    r[10] = r[11] = 0.3
    kinds = g.integers(0, 3, n).astype(np.int32)
    params = np.column_stack([g.uniform(0.1, 0.9, (n, 3)), np.where(kinds == 2, 1.5, g.uniform(0, 0.5, n))])
    cr = np.vstack([[0, -1000, 0, 1000], [0, 1, 40, 30], np.column_stack([c, r])])
    kinds = np.concatenate([[0, 1], kinds]).astype(np.int32)
    params = np.vstack([[0.5, 0.5, 0.5, 0], [0.7, 0.6, 0.5, 0.1], params])
    return rt.World(cr, kinds, params)


WORLDS = {}


def world_of(name):
    if name not in WORLDS:
        WORLDS[name] = rt.random_scene() if name == "final" else stacked_world()
    return WORLDS[name]


def cam_of(name, aspect):
    return rt.final_camera(aspect) if name == "final" else rt.camera((13, 4, 3), (0, 3, 0), (0, 1, 0), 40.0, aspect, 0.1, 10.0)


_RENDERERS = {}


@pytest.fixture(scope="module")
def renderers():
    """One context per (scene, memory); the global-memory ones are created
    with RTMI_GRID_GLOBAL=1 set, as tests/test_gpu_parity.py forces it."""
    mp = pytest.MonkeyPatch()

    def get(name, mem):
        if (name, mem) not in _RENDERERS:
            if mem == "global":
                mp.setenv("RTMI_GRID_GLOBAL", "1")
            try:
                r = rt.Renderer(world_of(name), 0)
            finally:
                mp.delenv("RTMI_GRID_GLOBAL", raising=False)
            r.set_kernel("grid")
            _RENDERERS[(name, mem)] = r
        return _RENDERERS[(name, mem)]

    yield get
    for r in _RENDERERS.values():
        r.close()
    _RENDERERS.clear()
    mp.undo()


_BRUTE = {}


def brute(get, name, key, fn):
    """The brute-force result of a case, rendered once (LDS context, no structure)."""
    if (name, key) not in _BRUTE:
        r = get(name, "lds")
        r.set_accel("none")
        try:
            _BRUTE[(name, key)] = fn(r)
        finally:
            r.set_accel("grid")
    return _BRUTE[(name, key)]


def grid_walk(name, mem):
    # render_rows_impl's kinds: 3 one layer, 2 general; + 2 in global memory
    # (last_schedule reports 3 as 2 and 5 as 4)
    return 2 if mem == "lds" else 4


def check_case(get, name, mem, key, fn, tile_w=0):
    want = brute(get, name, key, fn)
    r = get(name, mem)
    r.set_accel("grid")
    ny = r.grid_info()[0][1]
    assert (ny == 1) == (name == "final"), ny
    r.set_tuning(tile_w, 0)
    try:
        got = fn(r)
        sch = r.last_schedule()
    finally:
        r.set_tuning(0, 0)
    assert sch["bvh"] == grid_walk(name, mem) and sch["persistent"] == 0, sch
    if tile_w:
        assert sch["tile_w"] == tile_w, sch
    assert np.array_equal(got, want), f"{int((got != want).any(axis=-1).sum())} pixels differ"
    assert np.isfinite(got).all() and got.max() > 0


@pytest.mark.parametrize("mem", ["lds", "global"])
@pytest.mark.parametrize("name", ["final", "stacked"])
@pytest.mark.parametrize("tile_w", [8, 16])
@pytest.mark.parametrize("W,H", SIZES)
def test_images_with_full_and_partial_tiles(W, H, tile_w, name, mem, renderers):
    """37 x 19 and 100 x 13 at 5 spp, depth 6: tiles of 8 x 8 and 16 x 4 leave
    full tiles and partial ones (in x, in y and in both) in one image, so the
    job decode runs with 64 and with fewer valid pixels per tile."""
    cam = cam_of(name, W / H)
    check_case(renderers, name, mem, ("img", W, H), lambda r: r.render(cam, W, H, 5, 6, SEED), tile_w)


@pytest.mark.parametrize("mem", ["lds", "global"])
@pytest.mark.parametrize("name", ["final", "stacked"])
def test_strip_of_every_third_row(name, mem, renderers):
    """Rows 1, 4, 7, ... of the 37 x 19 image (row_step 3): the pixel index the
    generator is keyed by comes from row0 + row * row_step."""
    W, H = SIZES[0]
    cam = cam_of(name, W / H)
    nrows = (H - 1 + 2) // 3
    check_case(renderers, name, mem, ("strip", W, H),
               lambda r: r.progressive(cam, W, H, 5, 5, 6, SEED, row0=1, row_step=3, nrows=nrows))


@pytest.mark.parametrize("mem", ["lds", "global"])
@pytest.mark.parametrize("name", ["final", "stacked"])
def test_max_depth_one(name, mem, renderers):
    """max_depth 1: every path ends in its batch pass (sky or black)."""
    W, H = SIZES[1]
    cam = cam_of(name, W / H)
    check_case(renderers, name, mem, ("d1", W, H), lambda r: r.render(cam, W, H, 5, 1, SEED))


def grid_box(world):
    """(cells per axis, origin, cell size) of the scene's grid as the walk reads
    them (float32), from the host-only layout entry point."""
    L = rt.load()
    L.rt_debug_grid_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    L.rt_debug_grid_layout.restype = C.c_int
    sc = world.c_struct()
    dims, strides, box = (C.c_int32 * 3)(), (C.c_uint32 * 2)(), (C.c_float * 6)()
    assert L.rt_debug_grid_layout(C.byref(sc), dims, strides, box) == 0
    return np.array(dims), np.array(box[:3], np.float32), np.array(box[3:], np.float32)


def constructed_rays(world):
    """About 4 000 rays aimed at the prologue's cases, float32 [n, 6]."""
    n, g0, h = grid_box(world)
    g0, h = g0.astype(np.float64), h.astype(np.float64)
    g1 = g0 + n * h
    g = np.random.default_rng(23)
    rays = []

    def inside(m):
        return g0 + g.random((m, 3)) * (g1 - g0)

    def face(c, ax):  # the float32 face coordinate g0 + c*h the walk computes
        return float(np.float32(np.float32(c) * np.float32(h[ax]) + np.float32(g0[ax])))

    # 1. origins beyond each of the six faces, aimed at points inside the box
    #    and along the axis; the grid's y extent may lie inside the ground, so
    #    the far origins are only a few cells out
    for ax in range(3):
        for side in (0, 1):
            m = 150
            o = inside(m)
            o[:, ax] = (g0[ax] - g.uniform(0.01, 3, m)) if side == 0 else (g1[ax] + g.uniform(0.01, 3, m))
            d = inside(m) - o
            d[: m // 3] = 0.0
            d[: m // 3, ax] = 1.0 if side == 0 else -1.0
            rays.append(np.column_stack([o, d]))
    # 2. origins inside, random directions and directions along each axis with
    #    +0.0, -0.0 and +-1e-25 in the other components
    m = 600
    o = inside(m)
    d = g.normal(size=(m, 3))
    rays.append(np.column_stack([o, d]))
    small = np.array([0.0, -0.0, 1e-25, -1e-25])
    for ax in range(3):
        for sgn in (1.0, -1.0):
            m = 160
            o = inside(m)
            d = small[g.integers(0, 4, (m, 3))]
            d[:, ax] = sgn * g.choice([1.0, 0.3, 7.0], m)
            rays.append(np.column_stack([o, d]))
    # 3. origins exactly on cell faces (one, two or three coordinates), any direction
    m = 600
    o = inside(m)
    for k in range(m):
        for ax in range(3):
            if g.random() < 0.5:
                o[k, ax] = face(int(g.integers(0, n[ax] + 1)), ax)
    d = g.normal(size=(m, 3))
    z = g.random((m, 3)) < 0.15
    d[z] = small[g.integers(0, 4, int(z.sum()))]
    rays.append(np.column_stack([o, d]))
    # 4. rays that enter at the last (and the first) cell of each axis: from
    #    outside through the far corner cells, and from inside them outward and inward
    for ax in range(3):
        for last in (True, False):
            m = 130
            tgt = inside(m)
            c = n[ax] - 1 if last else 0
            tgt[:, ax] = g0[ax] + (c + g.random(m)) * h[ax]
            o = tgt.copy()
            other = (ax + 1 + g.integers(0, 2, m)) % 3
            o[np.arange(m), other] += g.choice([-1.0, 1.0], m) * (g1 - g0)[other] * g.uniform(1.0, 1.5, m)
            rays.append(np.column_stack([o, tgt - o]))
            o2 = tgt.copy()
            d2 = g.normal(size=(m, 3))
            rays.append(np.column_stack([o2, d2]))
    rays = np.vstack(rays)
    dz = np.all(rays[:, 3:] == 0, axis=1)
    rays[dz, 3:] = [0, -1, 0]  # no zero directions (not a ray)
    return np.ascontiguousarray(rays.astype(np.float32))


@pytest.mark.parametrize("mem", ["lds", "global"])
@pytest.mark.parametrize("name", ["final", "stacked"])
def test_constructed_rays_equal_brute_force(name, mem, renderers):
    """Hit index and t of every constructed ray equal the brute-force loop's
    bit for bit, for the one-layer and the general walk, in LDS and in global
    memory (walk kinds 3, 2, 5, 4)."""
    world = world_of(name)
    rays = constructed_rays(world)
    m = len(rays)
    assert 3500 <= m <= 6000, m
    r = renderers(name, mem)
    r.set_accel("grid")
    L = rt.load()
    L.rt_ctx_debug_hits.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    idx = np.zeros(2 * m, np.int32)
    t = np.zeros(2 * m, np.float32)
    rc = L.rt_ctx_debug_hits(r._h, rays.ctypes.data_as(C.POINTER(C.c_float)), m, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                             t.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0
    idx, t = idx.reshape(m, 2), t.reshape(m, 2)
    # the premise: a good part of the rays hit something other than the ground (index 0)
    assert (idx[:, 0] >= 1).mean() > 0.1, (idx[:, 0] >= 1).mean()
    bad = np.nonzero((idx[:, 0] != idx[:, 1]) | (t[:, 0].view(np.uint32) != t[:, 1].view(np.uint32)))[0]
    assert bad.size == 0, f"{bad.size} rays differ, first {rays[bad[0]]} idx {idx[bad[0]]} t {t[bad[0]]}"
