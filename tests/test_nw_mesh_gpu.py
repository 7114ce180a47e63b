"""Triangles in the Next-Week renderer on the GPU: the gfx950 kernels'
hit_triangle / make_rec against the plain C++ restatement
(tests/native/nw_mesh_ref.cpp, itself checked on the CPU by
tests/test_nw_mesh.py) bit for bit — closest hits through the uniform grid and
the BVH, from LDS and from global memory, watertightness, whole paths — and
the image invariants (grid == BVH, chunk splits, strips, persistent ==
one-shot), two ties to the existing oracle (hidden triangles change nothing; a
quad of two triangles renders as the rectangle), and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd.nextweek as nw
import nw_mesh_util as M
import oracle_py as O
from conftest import record_parity_stats

pytestmark = pytest.mark.gpu
SEED = 1984
SPHERES = [((2.5, -0.2, 0.9), 0.9), ((-1.9, -0.2, 0.9), 0.9), ((0.3, 2.0, 0.9), 0.8), ((0.3, -0.2, 3.1), 0.9),
           ((0.3, -0.2, 0.9), 0.6)]  # the last one inside the mesh


def scene_a(subdiv=2, spheres=True, instance=False, mats="plain", ground=False):
    """The icosphere of 20 * 4**subdiv triangles (+ 5 spheres).  mats "plain":
    one lambertian; "mixed": the triangles in four materials — lambertian,
    metal, dielectric and an image-textured lambertian; "light": the last
    quarter emits instead."""
    s = nw.Scene()
    grey = s.lambertian(s.solid(0.6, 0.5, 0.4))
    v, f = M.icosphere(subdiv)
    if mats == "plain":
        parts = [s.mesh(v, f, mat=grey)]
    else:
        img = np.random.default_rng(5).integers(0, 256, (8, 8, 3)).astype(np.uint8)
        last = s.diffuse_light(s.solid(4, 4, 3)) if mats == "light" else s.lambertian(s.image(img))
        ms = [grey, s.metal(s.solid(0.8, 0.8, 0.9), 0.3), s.dielectric(1.5), last]
        q = len(f) // 4
        parts = [s.mesh(v, f[k * q:(k + 1) * q], mat=ms[k]) for k in range(4)]
    mesh = s.group(parts)
    if instance:
        mesh = s.translate(s.rotate_y(mesh, 30), (0.4, 0.3, -0.5))
    s.add(mesh)
    if spheres:
        sm = [grey, s.metal(s.solid(0.7, 0.6, 0.5), 0.0), s.dielectric(1.5), grey, s.lambertian(s.solid(0.9, 0.2, 0.2))]
        for (c, r), m in zip(SPHERES, sm):
            s.add(s.sphere(c, r, m))
    if ground:
        s.add(s.sphere((0, -1002, 0), 1000, s.lambertian(s.checker(s.solid(0.2, 0.3, 0.1), s.solid(0.9, 0.9, 0.9)))))
    s.set_background(0.7, 0.8, 1.0)
    return s


def scene_bounds(flat):
    obj, _ = M.flat_arrays(flat)
    kind = obj[:, 12].view(np.int32)
    pts = [obj[kind == 7][:, :9].reshape(-1, 3)]
    sp = obj[kind == 0]
    pts += [sp[:, :3] - sp[:, 3:4], sp[:, :3] + sp[:, 3:4]]
    pts = np.concatenate(pts).astype(np.float64)
    return pts.min(axis=0), pts.max(axis=0)


def hit_rays(flat, n, seed):
    """Origins uniform in twice the scene's bounds — the box about the same
    centre with twice the volume (each extent x 2**(1/3)); normal directions
    with signed zeros and axis-aligned rays (M.signed_zero_rays).  With each
    extent doubled (8 x the volume) a sphere is hit by 14.5% of such rays and
    no arrangement of six of them by more than 18%, short of the 20% the tests
    below require of their ray sets."""
    lo, hi = scene_bounds(flat)
    c, h = (lo + hi) / 2, (hi - lo) / 2 * 2.0 ** (1.0 / 3.0)
    return M.signed_zero_rays(np.random.default_rng(seed), n, c - h, c + h)


def assert_hits_equal(s, rays, accels, min_hit=0.2):
    flat = s.flat()
    want_i, want_t = M.ref_closest(flat, rays)
    assert (want_i >= 0).mean() > min_hit, (want_i >= 0).mean()
    r = nw.NwRenderer(s)
    try:
        for accel in accels:
            r.set_accel(accel)
            assert r.accel_info()["accel"] == accel
            got_i, got_t, got_face = r.debug_hits(rays)
            for name, a, b in (("index", got_i, want_i), ("t", got_t.view(np.int32), want_t.view(np.int32))):
                bad = np.nonzero(a != b)[0]
                assert bad.size == 0, f"{accel} {name}: {bad.size} rays differ, first {bad[:5]}: {a[bad[:5]]} vs {b[bad[:5]]}"
            assert (got_face == -1).all()
    finally:
        r.close()
    return want_i


# ---- 6. closest hits, bit for bit -------------------------------------------
@pytest.mark.parametrize("instance", [False, True])
def test_hits_small_mesh_and_spheres_grid_then_bvh(instance):
    """(a) 320 triangles + 5 spheres, 200 000 rays, through the grid (staged in
    LDS) and the BVH; once with the mesh under rotate_y(30) + translate."""
    s = scene_a(instance=instance)
    idx = assert_hits_equal(s, hit_rays(s.flat(), 200_000, 21 + instance), ["grid", "bvh"])
    obj, _ = M.flat_arrays(s.flat())
    kinds = obj[idx[idx >= 0], 12].view(np.int32)
    assert (kinds == 7).sum() > 10_000 and (kinds == 0).sum() > 10_000  # both kinds win


@pytest.mark.parametrize("subdiv,ntri", [(4, 5120), (5, 20480)])
def test_hits_large_meshes_bvh(subdiv, ntri):
    """(b) 5 120 and (c) 20 480 triangles (no grid of 65 535 references holds
    the latter), 100 000 rays through the BVH walked from global memory."""
    s = scene_a(subdiv, spheres=False)
    assert s.flat()["n_obj"] == ntri
    assert_hits_equal(s, hit_rays(s.flat(), 100_000, 30 + subdiv), ["bvh"])


# ---- 7. every kernel path is reached -----------------------------------------
@pytest.mark.parametrize("subdiv,accel,want", [
    (2, "grid", dict(persistent=1, grid=1, nodes_lds=False, objects_lds=True)),
    (2, "bvh", dict(persistent=1, grid=0, nodes_lds=True, objects_lds=True)),
    # 1 280 triangles: 1 163 nodes (37 KB) fit the two-blocks-per-CU budget, nodes + objects (104 KB) do not:
    # "nodes in LDS, objects global".  (5 120 triangles have 152 KB of nodes: past a CU's LDS, all global.)
    (3, "bvh", dict(persistent=1, grid=0, nodes_lds=True, objects_lds=False)),
    (3, "grid", dict(persistent=1, grid=1, nodes_lds=False, objects_lds=True)),
    (5, "bvh", dict(persistent=0, grid=0, nodes_lds=False, objects_lds=False)),
])
def test_kernel_paths_are_reached(subdiv, accel, want):
    W, H, spp = 64, 40, 8
    s = scene_a(subdiv, spheres=subdiv == 2, ground=True)
    cam = nw.camera((6, 2.5, 7), M.CENTRE, (0, 1, 0), 35, W / H, 0.0, 9.0)
    r = nw.NwRenderer(s)
    try:
        r.set_accel(accel)
        img = r.render(cam, W, H, spp, 50, SEED)
        k, st = r.last_kernel(), r.last_staging()
        assert {"persistent": k["persistent"], "grid": k["grid"], **st} == want, (k, st)
        assert k["spheres_only"] == 0
        assert np.isfinite(img).all() and img.std() > 0
        # every path of one mesh renders the same image (kept across the parametrised cases)
        first = _PATH_IMAGES.setdefault(subdiv, img)
        assert np.array_equal(img, first), f"{accel}: max |d| {np.abs(img - first).max()}"
    finally:
        r.close()


_PATH_IMAGES = {}


# ---- 8. watertight on the device ----------------------------------------------
def test_device_walks_are_watertight():
    v, f = M.icosphere(2)
    s = nw.Scene()
    s.add(s.mesh(v, f, mat=s.lambertian(s.solid(0.5, 0.5, 0.5))))
    rays = np.zeros((150_000 + 2 * 162 + 480 + 6, 7), np.float32)
    rays[:, :6] = M.watertight_rays(v, f)
    want_i, want_t = M.ref_closest(s.flat(), rays)
    r = nw.NwRenderer(s)
    try:
        for accel in ("grid", "bvh"):
            r.set_accel(accel)
            assert r.accel_info()["accel"] == accel
            idx, t, _ = r.debug_hits(rays)
            assert (idx < 0).sum() == 0, (accel, np.nonzero(idx < 0)[0][:10])
            assert np.array_equal(idx, want_i) and np.array_equal(t.view(np.int32), want_t.view(np.int32)), accel
    finally:
        r.close()


# ---- 9. whole paths ------------------------------------------------------------
def test_traced_paths_equal_reference_segment_by_segment():
    """200 (pixel, sample) traces at depth 50 through spheres and lambertian,
    metal, glass and emitting triangles: every segment's winner, t and normal
    — and the next segment's origin, the record's point — are the checker's
    for that segment's (o, d), bit for bit."""
    W, H = 48, 32
    s = scene_a(mats="light", ground=True)
    flat = s.flat()
    obj, _ = M.flat_arrays(flat)
    kinds = obj[:, 12].view(np.int32)
    cam = nw.camera((6, 2.5, 7), M.CENTRE, (0, 1, 0), 35, W / H, 0.0, 9.0)
    g = np.random.default_rng(9)
    r = nw.NwRenderer(s)
    longest, ends_on_triangle, nseg = 0, 0, 0
    try:
        for _ in range(200):
            i, j, smp = int(g.integers(8, W - 8)), int(g.integers(6, H - 4)), int(g.integers(0, 64))
            seg, ids = r.debug_trace(cam, W, H, i, j, smp, max_depth=50, seed=SEED, cap=64)
            assert len(seg) >= 1
            rays = np.zeros((len(seg), 8), np.float32)
            rays[:, :6] = seg[:, :6]
            want_i, want_t = M.ref_closest(flat, rays)
            assert np.array_equal(ids[:, 0], want_i), (i, j, smp, ids[:, 0], want_i)
            for k in range(len(seg)):
                if want_i[k] < 0:
                    continue
                assert seg[k, 6].view(np.int32) == want_t[k].view(np.int32), (i, j, smp, k)
                p, n, _ = M.ref_record(flat, want_i[k], seg[k, :3], seg[k, 3:6], want_t[k])
                assert np.array_equal(seg[k, 7:10].view(np.int32), n.view(np.int32)), (i, j, smp, k, seg[k, 7:10], n)
                if k + 1 < len(seg):  # the next segment starts at the record's point
                    assert np.array_equal(seg[k + 1, :3].view(np.int32), p.view(np.int32)), (i, j, smp, k)
            longest = max(longest, len(seg))
            nseg += len(seg)
            ends_on_triangle += int(ids[-1, 0] >= 0 and kinds[ids[-1, 0]] == 7)
    finally:
        r.close()
    assert longest >= 3 and ends_on_triangle >= 1, (longest, ends_on_triangle, nseg)


# ---- 10. image invariants --------------------------------------------------------
W10, H10, SPP10 = 64, 40, 70


def _render_a(accel="bvh", env=None, monkeypatch=None, rows=None):
    for k, val in (env or {}).items():
        monkeypatch.setenv(k, val)  # read when the context is created
    s = scene_a(mats="mixed", ground=True)
    cam = nw.camera((6, 2.5, 7), M.CENTRE, (0, 1, 0), 35, W10 / H10, 0.0, 9.0)
    r = nw.NwRenderer(s)
    try:
        r.set_accel(accel)
        assert r.accel_info()["accel"] == accel
        if rows is None:
            img = r.render(cam, W10, H10, SPP10, 50, SEED)
        else:
            import torch

            row0, step, nrows = rows
            strip = torch.full((nrows, W10, 3), -1.0, dtype=torch.float32, device="cuda")
            st = torch.cuda.Stream()
            r.render_rows(cam, W10, H10, SPP10, 50, SEED, row0, step, nrows, strip.data_ptr(), st.cuda_stream)
            st.synchronize()
            img = strip.cpu().numpy()
        return img, r.last_kernel()
    finally:
        r.close()


@pytest.fixture(scope="module")
def base_image():
    img, k = _render_a("bvh")
    assert k["persistent"] == 1 and np.isfinite(img).all()
    return img


def test_image_grid_equals_bvh(base_image):
    img, k = _render_a("grid")
    assert k["grid"] == 1 and np.array_equal(img, base_image)


@pytest.mark.parametrize("accel", ["bvh", "grid"])
def test_image_chunk_splits(accel, base_image, monkeypatch):
    """The Next-Week path has no passes: 70 samples as one work item per tile
    and as two of 35 (RTMI_NW_CHUNK) — the automatic split is 32 + 32 + 6."""
    for chunk in ("70", "35"):
        img, k = _render_a(accel, {"RTMI_NW_CHUNK": chunk}, monkeypatch)
        assert k["chunk"] == int(chunk) and np.array_equal(img, base_image), chunk


@pytest.mark.parametrize("accel", ["bvh", "grid"])
def test_image_row_strips(accel, base_image):
    img, _ = _render_a(accel, rows=(1, 3, 14))  # rows 1, 4, ..., 37, then one past H: zero
    assert np.array_equal(img[:13], base_image[1::3]) and (img[13] == 0).all()


@pytest.mark.parametrize("accel", ["bvh", "grid"])
def test_image_persistent_equals_one_shot(accel, base_image, monkeypatch):
    img, k = _render_a(accel, {"RTMI_NW_PERSIST": "0"}, monkeypatch)
    assert k["persistent"] == 0 and np.array_equal(img, base_image)


def test_image_texture_reads_the_barycentric_uv():
    """One image-textured lambertian triangle under a white background, one
    sample per pixel, depth 2: a pixel whose camera ray hits it is exactly the
    texel at the checker's (u, v) = (V / det, W / det) of that ray
    (image_texture::value restated below); every other pixel is white."""
    W, H = 32, 20
    img = np.random.default_rng(8).integers(1, 256, (8, 8, 3)).astype(np.uint8)
    s = nw.Scene()
    s.add(s.rotate_y(s.triangle((-2, -1.5, 0), (2, -1.5, 0.5), (0, 2, -0.5), s.lambertian(s.image(img))), 20))
    s.set_background(1, 1, 1)
    flat = s.flat()
    cam = nw.camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40, W / H, 0.0, 5.0)
    r = nw.NwRenderer(s)
    one, f255 = np.float32(1), np.float32(255)
    hits = 0
    try:
        got = r.render(cam, W, H, 1, 2, SEED)
        for j in range(H):
            for i in range(W):
                seg, ids = r.debug_trace(cam, W, H, i, j, 0, max_depth=2, seed=SEED)
                want = np.ones(3, np.float32)
                if ids[0, 0] == 0:
                    hits += 1
                    _, _, uv = M.ref_record(flat, 0, seg[0, :3], seg[0, 3:6], seg[0, 6])
                    u = np.clip(uv[0], np.float32(0), one)
                    v = one - np.clip(uv[1], np.float32(0), one)
                    ti, tj = min(int(u * np.float32(8)), 7), min(int(v * np.float32(8)), 7)
                    ti = (ti + 8 // 2 + 8 // 3) % 8
                    want = (one / f255) * img[tj, ti].astype(np.float32)
                assert np.array_equal(got[j, i], want), (i, j, got[j, i], want)
    finally:
        r.close()
    assert hits > W * H // 5


# ---- 11. triangles that cannot be seen change nothing ------------------------------
def _hidden_triangles(s, lo, hi, n=500, seed=4):
    g = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    size = (hi - lo).min() * 0.08
    c = lo + size + (hi - lo - 2 * size) * g.random((n, 3))
    v = (c[:, None, :] + size * (g.random((n, 3, 3)) - 0.5) * 2).reshape(-1, 3)
    s.add(s.mesh(v, np.arange(3 * n, dtype=np.int32).reshape(-1, 3), mat=s.metal(s.solid(1, 1, 1), 0.0)))


@pytest.mark.parametrize("accel", ["bvh", "grid"])
@pytest.mark.parametrize("which", [2, 6])
def test_unreachable_triangles_change_nothing(which, accel):
    """500 triangles no path can reach leave the oracle's image of the
    untouched preset, bit for bit.  How they are out of reach:
    two_spheres (2): inside the upper lambertian sphere (centre (0, 10, 0),
    radius 10), within 4 of its centre — every ray starts outside or on the
    sphere and its first hit is the sphere; a scattered ray leaves along n +
    (a vector in the unit ball), never inward.
    cornell_box (6): below the floor, x, z in [100, 455], y in [-1000, -400].
    Ray origins are the camera and surface points inside the room's hull;
    normals never flip, so walls at x = 555, y = 555, z = 555 and the floor
    scatter away from the region, every other surface point lies above the
    floor's footprint, whose rectangle any segment down to the region crosses,
    and camera rays (slope <= tan 20 deg from (278, 278, -800)) stay above
    y = -215 until z = 555."""
    W, H, spp = 29, 23, 3
    s, cam = nw.preset(which, aspect=W / H)
    want, _ = O.nw_render(s.flat(), cam, W, H, spp, 50, SEED)
    if which == 2:
        _hidden_triangles(s, (-2.3, 7.7, -2.3), (2.3, 12.3, 2.3))
    else:
        _hidden_triangles(s, (100, -1000, 100), (455, -400, 455))
    assert s.flat()["n_obj"] >= 502
    r = nw.NwRenderer(s)
    try:
        r.set_accel(accel)
        if r.accel_info()["accel"] != accel:
            pytest.fail(f"scene {which}: no {accel}")
        got = r.render(cam, W, H, spp, 50, SEED)
    finally:
        r.close()
    assert np.array_equal(got, want), f"max |d| {np.abs(got - want).max()}"


# ---- 12. a quad is a quad ------------------------------------------------------------
def _cornell_triangles():
    """cornell_box (rt_nw_scene_preset case 6) with every rectangle — five
    walls and the light — as two triangles wound so that their normal is the
    rectangle's (+x, +y or +z: the renderer never flips normals)."""
    s = nw.Scene()
    red, white, green = (s.lambertian(s.solid(*c)) for c in ((.65, .05, .05), (.73, .73, .73), (.12, .45, .15)))
    light = s.diffuse_light(s.solid(15, 15, 15))

    def quad(plane, a0, a1, b0, b1, k, mat):
        if plane == "yz":
            p = [(k, a0, b0), (k, a1, b0), (k, a1, b1), (k, a0, b1)]  # y then z: normal +x
        elif plane == "xz":
            p = [(a0, k, b0), (a0, k, b1), (a1, k, b1), (a1, k, b0)]  # z then x: normal +y
        else:
            p = [(a0, b0, k), (a1, b0, k), (a1, b1, k), (a0, b1, k)]  # x then y: normal +z
        s.add(s.triangle(p[0], p[1], p[2], mat))
        s.add(s.triangle(p[0], p[2], p[3], mat))

    quad("yz", 0, 555, 0, 555, 555, green)
    quad("yz", 0, 555, 0, 555, 0, red)
    quad("xz", 213, 343, 227, 332, 554, light)
    quad("xz", 0, 555, 0, 555, 0, white)
    quad("xz", 0, 555, 0, 555, 555, white)
    quad("xy", 0, 555, 0, 555, 555, white)
    s.add(s.translate(s.rotate_y(s.box((0, 0, 0), (165, 330, 165), white), 15), (265, 0, 295)))
    s.add(s.translate(s.rotate_y(s.box((0, 0, 0), (165, 165, 165), white), -18), (130, 0, 65)))
    s.set_background(0, 0, 0)
    return s


def test_cornell_walls_as_triangle_pairs_match_the_rectangles():
    """200 x 200 x 256: the per-channel image means of the triangle build lie
    within 5 standard errors of the rectangle build's, the standard error
    being the spread of the rectangle build's own means over 8 seeds."""
    W = H = 200
    spp = 256
    s_rect, cam = nw.preset(6, aspect=1.0)
    s_tri = _cornell_triangles()
    tri = M.flat_triangles(s_tri.flat()).reshape(-1, 3, 3).astype(np.float64)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert len(tri) == 12 and (nrm >= 0).all() and ((nrm > 0).sum(axis=1) == 1).all()
    r = nw.NwRenderer(s_rect)
    try:
        means = np.array([r.render(cam, W, H, spp, 50, SEED + k).mean(axis=(0, 1)) / spp for k in range(8)])
        r.set_scene(s_tri)
        got = r.render(cam, W, H, spp, 50, SEED + 100).mean(axis=(0, 1)) / spp
    finally:
        r.close()
    mean, se = means.mean(axis=0), means.std(axis=0, ddof=1)
    z = (got - mean) / se
    print(f"cornell rect means {mean} se {se}; triangles {got}; z {z}")
    record_parity_stats("nw_mesh_cornell_quads", {f"{n}_{c}": v for n, a in (("rect_mean", mean), ("rect_se", se),
                                                                             ("tri_mean", got), ("z", z))
                                                  for c, v in zip("rgb", a.tolist())})
    assert (np.abs(z) <= 5).all(), z


# ---- 13. the CLI ----------------------------------------------------------------------
@pytest.mark.parametrize("mat", ["lambertian", "glass"])
def test_cli_obj_matches_library(tmp_path, mat):
    exe = os.path.join(os.path.dirname(nw.__file__), "bin", "rtmi_nw_render")
    path = tmp_path / "cube.obj"
    path.write_text(M.cube_obj("a//n", quads=True, scale=3.0, offset=(5.0, -2.0, 1.0)))
    W, H, spp = 24, 16, 4
    out = tmp_path / "o.ppm"
    subprocess.run([exe, "--obj", str(path), "--obj-mat", mat, "--width", str(W), "--height", str(H), "--spp", str(spp),
                    "--out", str(out)], check=True, capture_output=True, timeout=120)
    tok = out.read_text().split()
    assert tok[:4] == ["P3", str(W), str(H), "255"]
    got = np.array(tok[4:], np.int64).reshape(H, W, 3)
    s, cam, n = nw.obj_stage(path, mat, aspect=W / H)
    assert n == 12
    tris = M.flat_triangles(s.flat()).reshape(-1, 3)
    assert np.allclose(tris.min(axis=0), [-1, 0, -1]) and np.allclose(tris.max(axis=0), [1, 2, 1])  # the 2-unit box
    r = nw.NwRenderer(s)
    sums = r.render(cam, W, H, spp, 50, SEED)
    r.close()
    mean = (sums / np.float32(spp)).astype(np.float32)
    want = np.floor(255.99 * np.sqrt(mean).astype(np.float32).astype(np.float64)).astype(np.int64)[::-1]
    assert np.array_equal(got, want)
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 20  # a picture, not a flat colour
    p = subprocess.run([exe, "--obj", str(path), "--scene", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "exclusive" in p.stderr
