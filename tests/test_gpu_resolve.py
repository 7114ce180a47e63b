"""The one-root hit acceptance (csrc/rtmi_accept.h through resolve_root and
resolve_key) and the one-layer DDA step that recomputes both face parameters
(DESIGN.md §4.5).  Every case is grid == brute force or BVH == brute force,
bit for bit on the same device: images with full and partial tiles at tile
widths 8 and 16 and at max_depth 1, on the final scene (the one-layer walk
and its tile lists) and on a scene stacked in y that also holds two identical
big spheres (ties in resolve_root), two identical small spheres in one cell,
one small sphere on a cell corner (tested again from several cells with
t == t_max and its own key) and hollow shells with r < 0, with the structure
in LDS and in global memory; and constructed rays through rt_ctx_debug_hits:
origins inside spheres and shells (r1 < 0.001 <= r2), origins stepped in
single ulps across the distance that puts r1 on either side of 0.001, tangent
rays with disc = 0 and with disc so small that sqrt_cr takes its guard's
path, spheres wholly behind the origin, rays through both coincident pairs
from both sides, rays along the whole grid in +x, -x, +z and -z (k reaches
kmax), diagonals through cell corners (tnx == tnz), and the prologue test's
rays (axis-parallel with +0.0, -0.0 and 1e-25 components, entering at the
last cell of each axis)."""
import ctypes as C

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd as rt
from test_gpu_prologue import constructed_rays as prologue_rays
from test_gpu_prologue import grid_box

pytestmark = pytest.mark.gpu

SEED = 1984
SIZES = [(37, 19), (100, 13)]
SPP, DEPTH = 8, 50

# scene indices of the constructed spheres of stacked_world()
GROUND, BIG_A, BIG_B, TWIN_A, TWIN_B, SHELL_OUT, SHELL_IN, TANGENT_SMALL, TANGENT_BIG, CORNER = range(10)
N_FIXED = 10


def stacked_world():
    """240 random spheres stacked in y (several cell layers, 4 % of them with
    r < 0) behind ten constructed ones: the ground, two identical big spheres,
    two identical small ones, a hollow shell (r = 0.4 around r = -0.35), a
    small and a big sphere at dyadic coordinates (exact tangents), and a small
    sphere that corner_on_cell_faces() moves onto a cell corner."""
    g = np.random.default_rng(11)
    n = 240
    c = g.uniform(-6, 6, (n, 3))
    c[:, 1] = g.uniform(-0.5, 7, n)
    r = np.exp(g.uniform(np.log(0.05), np.log(0.5), n))
    r[g.random(n) < 0.04] *= -1
    fixed = np.array([
        [0, -1000, 0, 1000],
        [1.5, 2.5, -1.0, 1.25], [1.5, 2.5, -1.0, 1.25],
        [-2.0, 3.0, 1.0, 0.15], [-2.0, 3.0, 1.0, 0.15],
        [3.0, 1.0, 2.5, 0.4], [3.0, 1.0, 2.5, -0.35],
        [2.0, 1.0, -3.0, 0.5],
        [-3.0, 4.0, -2.0, 1.0],
        [0.3, 3.1, 0.2, 0.5],
    ])
    kinds = np.concatenate([[0, 2, 1, 0, 1, 2, 2, 0, 1, 0], g.integers(0, 3, n)]).astype(np.int32)
    params = np.column_stack([g.uniform(0.1, 0.9, (N_FIXED + n, 3)), np.where(kinds == 2, 1.5, g.uniform(0, 0.5, N_FIXED + n))])
    return rt.World(np.vstack([fixed, np.column_stack([c, r])]), kinds, params)


def corner_on_cell_faces(world):
    """The same world with sphere CORNER centred on an inner cell corner of the
    grid (its box and cell size do not depend on that sphere: it lies well
    inside the others' extent)."""
    n, g0, h = grid_box(world)
    cr = np.array(world.center_radius, np.float64).reshape(-1, 4).copy()
    cell = np.maximum(n // 2, 1)
    cr[CORNER, :3] = g0.astype(np.float64) + cell * h.astype(np.float64)
    w = rt.World(cr, np.array(world.mat_kind, np.int32), np.array(world.mat_params, np.float64).reshape(-1, 4))
    n2, g02, h2 = grid_box(w)
    assert np.array_equal(n, n2) and np.array_equal(g0, g02) and np.array_equal(h, h2)
    return w


WORLDS = {}


def world_of(name):
    if name not in WORLDS:
        WORLDS[name] = rt.random_scene() if name == "final" else corner_on_cell_faces(stacked_world())
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
            assert r.last_schedule()["bvh"] == 0
        finally:
            r.set_accel("grid")
    return _BRUTE[(name, key)]


def check_case(get, name, mem, key, fn, tile_w=0):
    """mem: "lds" / "global" the grid in that memory, "bvh" the BVH."""
    want = brute(get, name, key, fn)
    r = get(name, "lds" if mem == "bvh" else mem)
    r.set_accel("bvh" if mem == "bvh" else "grid")
    r.set_tuning(tile_w, 0)
    try:
        ny = r.grid_info()[0][1]
        assert (ny == 1) == (name == "final"), ny
        got = fn(r)
        sch = r.last_schedule()
    finally:
        r.set_tuning(0, 0)
        r.set_accel("grid")
    # render_rows_impl's kinds as last_schedule reports them: 1 BVH, 2 the grid in LDS, 4 in global memory
    assert sch["bvh"] == {"bvh": 1, "lds": 2, "global": 4}[mem] and sch["persistent"] == 0, sch
    if tile_w:
        assert sch["tile_w"] == tile_w, sch
    assert np.array_equal(got, want), f"{int((got != want).any(axis=-1).sum())} pixels differ"
    assert np.isfinite(got).all() and got.max() > 0


@pytest.mark.parametrize("mem", ["lds", "global"])
@pytest.mark.parametrize("name", ["final", "stacked"])
@pytest.mark.parametrize("tile_w", [8, 16])
@pytest.mark.parametrize("W,H", SIZES)
def test_images_grid_equals_brute_force(W, H, tile_w, name, mem, renderers):
    """37 x 19 and 100 x 13 at 8 spp, depth 50, tiles of 8 x 8 and 16 x 4."""
    cam = cam_of(name, W / H)
    check_case(renderers, name, mem, ("img", W, H), lambda r: r.render(cam, W, H, SPP, DEPTH, SEED), tile_w)


@pytest.mark.parametrize("name", ["final", "stacked"])
@pytest.mark.parametrize("W,H", SIZES)
def test_images_bvh_equals_brute_force(W, H, name, renderers):
    """The BVH walk resolves through resolve_root: the same images."""
    cam = cam_of(name, W / H)
    check_case(renderers, name, "bvh", ("img", W, H), lambda r: r.render(cam, W, H, SPP, DEPTH, SEED))


def test_final_scene_with_tile_lists(renderers):
    """16 spp: the least at which the automatic four items per tile build their
    lists (kTileListMinSpp = 4), so the batch passes resolve through the list loop."""
    W, H = SIZES[0]
    cam = cam_of("final", W / H)
    check_case(renderers, "final", "lds", ("img16", W, H), lambda r: r.render(cam, W, H, 16, DEPTH, SEED))


@pytest.mark.parametrize("mem", ["lds", "global", "bvh"])
@pytest.mark.parametrize("name", ["final", "stacked"])
def test_max_depth_one(name, mem, renderers):
    """max_depth 1: every path ends in its batch pass (sky or black)."""
    W, H = SIZES[1]
    cam = cam_of(name, W / H)
    check_case(renderers, name, mem, ("d1", W, H), lambda r: r.render(cam, W, H, SPP, 1, SEED))


def ulp_steps(x, ks):
    """float32 x moved by each k of ks units in the last place."""
    b = np.float32(x).view(np.int32)
    assert b > 0
    return (b + np.asarray(ks, np.int32)).view(np.float32).astype(np.float64)


def resolve_rays(world, name):
    """A few thousand rays aimed at the acceptance and the step, float32 [n, 6]."""
    cr = np.array(world.center_radius, np.float64).reshape(-1, 4)
    n, g0, h = grid_box(world)
    g0, h = g0.astype(np.float64), h.astype(np.float64)
    g1 = g0 + n * h
    g = np.random.default_rng(29)
    rays = []

    def unit(m):
        v = g.normal(size=(m, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    med = np.median(np.abs(cr[:, 3]))
    big = [k for k in range(len(cr)) if abs(cr[k, 3]) > 4 * med]
    if name == "final":
        solid = big + list(g.choice(np.arange(1, len(cr)), 12, replace=False))
        pairs, shells = [], []
    else:
        solid = [GROUND, BIG_A, TWIN_A, TANGENT_SMALL, TANGENT_BIG, CORNER] + list(N_FIXED + g.choice(240, 6, replace=False))
        pairs, shells = [(BIG_A, BIG_B), (TWIN_A, TWIN_B)], [(SHELL_OUT, SHELL_IN)]
    # 1. origins inside a sphere (r1 < 0.001 <= r2), any direction; inside the ground only just below its top
    for k in solid:
        c, r = cr[k, :3], abs(cr[k, 3])
        m = 40
        o = c + unit(m) * (r * (1 - g.uniform(1e-4, 1e-2, (m, 1))) if k == GROUND else r * g.uniform(0, 0.999, (m, 1)))
        if k == GROUND:
            o = o[o[:, 1] > -1]  # near the scene
        rays.append(np.column_stack([o, g.normal(size=(len(o), 3))]))
    #    ... and inside a shell's wall (between the inner and the outer radius) and inside its hollow
    for ko, ki in shells:
        c, ro, ri = cr[ko, :3], abs(cr[ko, 3]), abs(cr[ki, 3])
        m = 120
        o = c + unit(m) * np.concatenate([g.uniform(ri, ro, (m // 2, 1)), g.uniform(0, ri, (m // 2, 1))])
        rays.append(np.column_stack([o, g.normal(size=(m, 3))]))
    # 2. along +x towards the centre from the distance that puts the near root at 0.001 (|d| = 1) or at
    #    0.001 with d twice as long, the origin's x stepped by single ulps through it
    for k in solid[1:7]:
        c, r = cr[k, :3], abs(cr[k, 3])
        for dlen, gap in ((1.0, 0.001), (2.0, 0.002), (0.5, 0.0005)):
            x0 = c[0] - (r + gap)
            if abs(x0) < 1e-3:
                continue
            xs = ulp_steps(abs(x0), np.arange(-48, 49)) * np.sign(x0)
            o = np.column_stack([xs, np.full(len(xs), c[1]), np.full(len(xs), c[2])])
            rays.append(np.column_stack([o, np.tile([dlen, 0.0, 0.0], (len(xs), 1))]))
    # 3. tangents along +x at y = c.y + r: with dyadic coordinates every term of the discriminant is exact
    #    and disc = 0; y stepped by ulps to either side gives a tiny disc of either sign; with d scaled by
    #    2^-40 and 2^-60 the positive ones fall below 2^-96 and into the denormals (sqrt_cr's guard)
    tang = [TANGENT_SMALL, TANGENT_BIG] if name != "final" else big[1:3]
    for k in tang:
        c, r = cr[k, :3], abs(cr[k, 3])
        ys = ulp_steps(c[1] + r, np.arange(-24, 9))
        for s in (1.0, 2.0 ** -40, 2.0 ** -60):
            o = np.column_stack([np.full(len(ys), c[0] - 6.0), ys, np.full(len(ys), c[2])])
            rays.append(np.column_stack([o, np.tile([s, 0.0, 0.0], (len(ys), 1))]))
    # 4. spheres wholly behind the origin: from just outside, pointing away
    for k in solid[1:]:
        c, r = cr[k, :3], abs(cr[k, 3])
        m = 30
        u = unit(m)
        o = c + u * r * g.uniform(1.001, 1.5, (m, 1))
        rays.append(np.column_stack([o, u + 0.3 * g.normal(size=(m, 3))]))
    # 5. through both coincident pairs (and the shell) from both sides, through the centre and off it
    for ka, _ in pairs + shells:
        c, r = cr[ka, :3], abs(cr[ka, 3])
        m = 100
        u = unit(m)
        off = unit(m) * r * g.uniform(0, 1.1, (m, 1)) * (g.random((m, 1)) < 0.7)
        for sgn in (1.0, -1.0):
            o = c + off + sgn * u * (r + g.uniform(0.5, 4, (m, 1)))
            rays.append(np.column_stack([o, -sgn * u * g.choice([1.0, 0.25, 3.0], (m, 1))]))
    # 6. the whole length of the grid along +x, -x, +z and -z, from outside and from the first cell,
    #    with +0.0, -0.0 and +-1e-25 in the other components
    small = np.array([0.0, -0.0, 1e-25, -1e-25])
    for ax in (0, 2):
        for sgn in (1.0, -1.0):
            m = 120
            o = g0 + g.random((m, 3)) * (g1 - g0)
            start = g0[ax] if sgn > 0 else g1[ax]
            o[:, ax] = start - sgn * np.where(g.random(m) < 0.5, g.uniform(0.01, 2, m), -g.uniform(0.0, 0.9, m) * h[ax])
            d = small[g.integers(0, 4, (m, 3))]
            d[:, ax] = sgn * g.choice([1.0, 0.3, 7.0], m)
            rays.append(np.column_stack([o, d]))
    # 7. diagonals in x, z through cell corners: from a corner along (+-h.x, 0, +-h.z), so that both
    #    faces come up at the same parameter
    m = 300
    cx, cz = g.integers(0, n[0] + 1, m), g.integers(0, n[2] + 1, m)
    o = np.column_stack([np.float32(np.float32(cx) * np.float32(h[0]) + np.float32(g0[0])), g0[1] + g.random(m) * (g1[1] - g0[1]),
                         np.float32(np.float32(cz) * np.float32(h[2]) + np.float32(g0[2]))])
    d = np.column_stack([g.choice([-1.0, 1.0], m) * h[0], small[g.integers(0, 4, m)], g.choice([-1.0, 1.0], m) * h[2]])
    d *= g.choice([1.0, 0.5, 2.0], (m, 1))
    rays.append(np.column_stack([o, d]))
    rays = np.vstack(rays).astype(np.float32)
    # 8. the prologue test's rays: beyond each face, on cell faces, axis-parallel, entering at the last cells
    return np.ascontiguousarray(np.vstack([rays, prologue_rays(world)]))


_RAYS = {}


@pytest.mark.parametrize("mem", ["lds", "global", "bvh"])
@pytest.mark.parametrize("name", ["final", "stacked"])
def test_constructed_rays_equal_brute_force(name, mem, renderers):
    """Hit index and t of every constructed ray equal the brute-force loop's bit
    for bit: the one-layer and the general walk, in LDS and in global memory,
    and the BVH."""
    world = world_of(name)
    if name not in _RAYS:
        _RAYS[name] = resolve_rays(world, name)
    rays = _RAYS[name]
    m = len(rays)
    assert 6000 <= m <= 14000, m
    r = renderers(name, "lds" if mem == "bvh" else mem)
    r.set_accel("bvh" if mem == "bvh" else "grid")
    L = rt.load()
    L.rt_ctx_debug_hits.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    idx = np.zeros(2 * m, np.int32)
    t = np.zeros(2 * m, np.float32)
    try:
        rc = L.rt_ctx_debug_hits(r._h, rays.ctypes.data_as(C.POINTER(C.c_float)), m, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                 t.ctypes.data_as(C.POINTER(C.c_float)))
    finally:
        r.set_accel("grid")
    assert rc == 0
    idx, t = idx.reshape(m, 2), t.reshape(m, 2)
    # the premise: a good part of the rays hit something other than the ground (index 0), and some miss
    assert (idx[:, 0] >= 1).mean() > 0.1, (idx[:, 0] >= 1).mean()
    assert (idx[:, 0] < 0).any()
    if name == "stacked":
        # ties decided for the later twin: the brute-force loop itself reports the second sphere of each pair
        assert (idx[:, 0] == BIG_B).sum() > 50 and (idx[:, 0] == TWIN_B).sum() > 20, ((idx[:, 0] == BIG_B).sum(), (idx[:, 0] == TWIN_B).sum())
        assert (idx[:, 0] == BIG_A).sum() == 0 and (idx[:, 0] == TWIN_A).sum() == 0
        assert (idx[:, 0] == SHELL_IN).sum() > 20
    bad = np.nonzero((idx[:, 0] != idx[:, 1]) | (t[:, 0].view(np.uint32) != t[:, 1].view(np.uint32)))[0]
    assert bad.size == 0, f"{bad.size} rays differ, first {rays[bad[0]]} idx {idx[bad[0]]} t {t[bad[0]]}"


def test_corner_sphere_spans_cells():
    """The premise of the stacked scene: several y layers, the two small twins
    in one cell, and the corner sphere in eight cells."""
    world = world_of("stacked")
    n, g0, h = grid_box(world)
    assert n[1] > 1, n
    cr = np.array(world.center_radius, np.float64).reshape(-1, 4)

    def cells(k):
        lo = np.floor((cr[k, :3] - abs(cr[k, 3]) - g0) / h).astype(int)
        hi = np.floor((cr[k, :3] + abs(cr[k, 3]) - g0) / h).astype(int)
        return int(np.prod(np.clip(hi, 0, n - 1) - np.clip(lo, 0, n - 1) + 1))

    assert cells(CORNER) == 8, cells(CORNER)
    assert np.array_equal(cr[TWIN_A], cr[TWIN_B]) and np.array_equal(cr[BIG_A], cr[BIG_B])
    med = np.median(np.abs(cr[:, 3]))
    assert cr[BIG_A, 3] > 4 * med and cr[TANGENT_BIG, 3] > 4 * med  # kept out of the grid: resolve_root
    assert cr[TANGENT_SMALL, 3] < 4 * med and cr[CORNER, 3] < 4 * med and cr[TWIN_A, 3] < 4 * med  # in the grid: resolve_key
