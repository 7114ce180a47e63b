"""Mesh images against the oracle, bit for bit: scenes in which paths touch
triangles — beside every other object kind of the Next-Week renderer — are
rendered by the gfx950 kernels' TRI = 1, 2 and 3 instantiations and compared
with oracle/rt_nw_oracle.inc (brute force over the flattened scene; its
triangle code is checked on the CPU by tests/test_nw_mesh_oracle.py): the
float sums with np.array_equal, the world.hit counts, closest hits, box faces
and hit records.  Every test asserts the kernel path it reached and, from the
oracle's winners by kind alone, that its paths meet what the test is about.
The scene, cameras and conditions: tests/nw_mixed_util.py."""
import os

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd.nextweek as nw
import nw_instance_util as U
import nw_mesh_util as M
import nw_mixed_util as X
import nw_smooth_util as S
import oracle_py as O

pytestmark = pytest.mark.gpu
SEED = X.SEED
SMALL, LARGE = (29, 23, 3), (24, 40, 70)  # partial 8 x 8 tiles on both axes; three work items per pixel
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _render(scene, cam, W, H, spp, accel, depth=50, seed=SEED):
    """(image, segments, last_kernel, last_staging, accel in use)."""
    r = nw.NwRenderer(scene)
    try:
        r.set_accel(accel)
        used = r.accel_info()["accel"]
        img = r.render(cam, W, H, spp, depth, seed)
        return img, r.last_segments(), r.last_kernel(), r.last_staging(), used
    finally:
        r.close()


def _assert_image(got, want, what=""):
    img, segs = got[0], got[1]
    assert segs == want[1], (what, segs, want[1])
    bad = np.nonzero((img != want[0]).any(axis=2))
    assert np.array_equal(img, want[0]), f"{what}: {len(bad[0])} pixels differ, first (row, col) {list(zip(*bad))[:5]}"


# what a render walks from LDS (rt_nw_ctx_last_staging).  The flattened mixed scene on the BVH: its 691 nodes (22 KB)
# are staged, nodes + 689 objects (58 KB) exceed both the two-blocks-per-CU budget and the one-shot kernel's 34 KB
GRID = {"nodes_lds": False, "objects_lds": True}          # the grid kernels stage the objects with the cells
NODES = {"nodes_lds": True, "objects_lds": False}
ALL_LDS = {"nodes_lds": True, "objects_lds": True}        # (shared meshes: the top level; the pool stays in global memory)


def _assert_path(got, accel, persistent, staging):
    _, _, k, st, used = got
    assert used == accel, (used, accel)
    assert (k["persistent"], k["grid"], k["spheres_only"]) == (persistent, int(accel == "grid"), 0), (k, st)
    assert st == staging, (k, st)


# ---- 1. TRI = 1 and TRI = 2 images ---------------------------------------------
# the one-shot grid kernel stages at most 34 KB per block — 52 B per object, so fewer than 670 objects — and the
# scene's two flattened copies of icosphere(2) alone are 642: that case keeps the in-place icosphere(2) and builds
# the copy under rotate_y + translate from icosphere(1)
@pytest.mark.parametrize("attr,accel,persist,size,second", [
    (a, acc, p, SMALL, 1 if (acc, p) == ("grid", "0") else 2) for a in (False, True) for acc in ("grid", "bvh") for p in ("1", "0")
] + [(True, "grid", "1", LARGE, 2), (True, "bvh", "1", LARGE, 2)])
def test_mixed_scene_images_equal_the_oracle(attr, accel, persist, size, second, monkeypatch):
    """The mixed scene, flattened (TRI = 1 without, TRI = 2 with attribute
    records), through the grid and the BVH, persistent and one-shot.
    Oracle's shares of the hitting segments (triangle, moving sphere,
    rectangle, box, medium) and of misses among all segments:
    (29, 23, 3)  flat .183 .098 .288 .082 .043, misses .223; with attributes .181 .098 .294 .079 .044, .222
    (29, 23, 3)  second copy from icosphere(1): flat .179 .101 .289 .080 .044, .222; with attributes .180 .100 .293 .077 .045, .221
    (24, 40, 70) with attributes .212 .057 .292 .073 .055, misses .235"""
    W, H, spp = size
    s = X.mixed_scene(False, attr, second)
    cam = X.mixed_camera(W, H)
    want = X.oracle_image(("mixed", False, attr, second, size), s, cam, W, H, spp)
    X.assert_mixed_conditions(want[2])
    assert (len(s.flat_attr()["attr"]) > 0) == attr
    monkeypatch.setenv("RTMI_NW_PERSIST", persist)  # read when the context is created
    got = _render(s, cam, W, H, spp, accel)
    _assert_path(got, accel, int(persist), GRID if accel == "grid" else NODES)
    _assert_image(got, want, f"attr {attr} {accel} persist {persist}")


# ---- 2. TRI = 3 images -----------------------------------------------------------
@pytest.mark.parametrize("size", [SMALL, LARGE])
@pytest.mark.parametrize("persist", ["1", "0"])
@pytest.mark.parametrize("attr", [False, True])
def test_shared_scene_images_equal_the_oracle_of_the_flat_view(attr, persist, size, monkeypatch):
    """The icosphere as one shared mesh placed three times (two placements
    coincide): the two-level walk's image is the oracle's of Scene.flat().  The
    third placement loses every tie to the second, so the oracle's shares are
    those of test_mixed_scene_images_equal_the_oracle."""
    W, H, spp = size
    s = X.mixed_scene(True, attr)
    st = s.instancing_stats()
    assert (st["meshes"], st["placements"], st["pool_triangles"]) == (1, 3, 320)
    assert s.flat()["n_obj"] == 3 * 321 + 20 + 29
    cam = X.mixed_camera(W, H)
    want = X.oracle_image(("mixed", True, attr, 2, size), s, cam, W, H, spp)
    X.assert_mixed_conditions(want[2])
    monkeypatch.setenv("RTMI_NW_PERSIST", persist)
    got = _render(s, cam, W, H, spp, "auto")
    _assert_path(got, "bvh", int(persist), ALL_LDS)
    _assert_image(got, want, f"shared attr {attr} persist {persist}")


# ---- 3. strips ---------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
def test_mixed_scene_row_strips_equal_the_oracle(shared):
    """render_rows on a torch stream: rows 1, 4, ..., 22 and one past H."""
    import torch

    W, H, spp = SMALL
    row0, step, nrows = 1, 3, 9  # rows 1 .. 22, then 25 >= H
    s = X.mixed_scene(shared, True)
    cam = X.mixed_camera(W, H)
    want = X.oracle_image(("strips", shared), s, cam, W, H, spp, row0=row0, row_step=step, nrows=nrows)
    assert (want[0][nrows - 1] == 0).all() and want[0][:nrows - 1].std() > 0
    whole = X.oracle_image(("mixed", shared, True, 2, SMALL), s, cam, W, H, spp)
    X.assert_mixed_conditions(whole[2])
    assert np.array_equal(want[0][:nrows - 1], whole[0][row0::step])
    r = nw.NwRenderer(s)
    try:
        r.set_accel("auto" if shared else "bvh")
        assert r.accel_info()["accel"] == "bvh"
        strip = torch.full((nrows, W, 3), -1.0, dtype=torch.float32, device="cuda")
        st = torch.cuda.Stream()
        r.render_rows(cam, W, H, spp, 50, SEED, row0, step, nrows, strip.data_ptr(), st.cuda_stream)
        st.synchronize()
        img = strip.cpu().numpy()
        k = r.last_kernel()
        assert (k["persistent"], k["grid"], k["spheres_only"]) == (1, 0, 0), k
        assert r.last_staging() == (ALL_LDS if shared else NODES)
        assert r.last_segments() == want[1]
    finally:
        r.close()
    assert np.array_equal(img, want[0]) and (img[nrows - 1] == 0).all()


# ---- 4. staging paths -----------------------------------------------------------------
def _one_icosphere(subdiv):
    def add(s):
        v, f = M.icosphere(subdiv)
        q = len(f) // 4
        image = s.lambertian(s.image(S.TEXTURE))
        ms = [s.lambertian(s.solid(0.6, 0.5, 0.4)), s.metal(s.solid(0.8, 0.8, 0.9), 0.3), s.dielectric(1.5), image]
        s.add(s.group([X._mesh(s, v, f[k * q:(k + 1) * q], ms[k], True, M.CENTRE, M.RADIUS) for k in range(4)]))
    return add


@pytest.mark.parametrize("subdiv,ntri,persistent,staging", [
    (3, 1280, 1, {"nodes_lds": True, "objects_lds": False}),
    (4, 5120, 0, {"nodes_lds": False, "objects_lds": False}),
])
def test_staging_paths_equal_the_oracle(subdiv, ntri, persistent, staging):
    """The mixed scene's other objects around one smooth icosphere of 1 280
    triangles (nodes in LDS, objects global) and of 5 120 (all global, the
    one-shot kernel), on the BVH, the camera turned to the icosphere.  Oracle
    at (24, 16, 2): triangles win .191 / .193 of the hitting segments, moving
    spheres .074 / .077, rectangles .29, boxes .095, media .017; misses .22."""
    W, H, spp = 24, 16, 2
    s = X.mixed_scene(False, True, mesh_only=_one_icosphere(subdiv))
    assert s.flat()["n_obj"] == ntri + 29
    cam = X.mixed_camera(W, H, lookat=(0.8, -0.4, 0.9), vfov=20.0)
    want = X.oracle_image(("staging", subdiv), s, cam, W, H, spp)
    X.assert_mixed_conditions(want[2])
    got = _render(s, cam, W, H, spp, "bvh")
    _assert_path(got, "bvh", persistent, staging)
    _assert_image(got, want, f"icosphere({subdiv})")


def _field_scene(shared):
    """nw_instance_util.field(shared, 5, 4) — icosphere(5) placed four times —
    with a box-bounded medium between the copies and a moving sphere."""
    s = U.field(shared, 5, 4)
    grey = s.lambertian(s.solid(0.5, 0.5, 0.5))
    s.add(s.constant_medium(s.box((1.2, -2.0, -1.0), (2.8, 1.5, 5.0), grey), 0.8, s.solid(0.9, 0.9, 0.9)))
    s.add(s.moving_sphere((2.0, 2.2, 2.0), (2.3, 2.8, 2.2), 0.0, 1.0, 0.8, s.metal(s.solid(0.8, 0.7, 0.6), 0.1)))
    s.set_background(0.7, 0.8, 1.0)
    return s


def test_large_shared_field_equals_the_oracle():
    """81 920 flat triangles as one bottom level of 20 480 (19 019 nodes, 594
    KB: far beyond a CU's LDS), four placements, a medium and a moving sphere:
    the two-level walk, its bottom level in global memory, == the oracle's
    brute force over the flat view.  Oracle at (24, 16, 1): of 724 segments
    383 miss (.53); triangles win 258 (.76 of the hitting ones), the medium
    63, the moving sphere 20."""
    W, H, spp = 24, 16, 1
    s = _field_scene(True)
    st = s.instancing_stats()
    assert (st["placements"], st["pool_triangles"]) == (4, 20480) and st["bottom_nodes"] * 32 > 160 * 1024
    assert s.flat()["n_obj"] == 81920 + 2
    cam = nw.camera((2.0, 4.0, 14.0), (2.0, -0.2, 2.0), (0, 1, 0), 26.0, W / H, 0.1, 12.5, 0.3, 0.6)
    want = X.oracle_image(("field",), s, cam, W, H, spp)
    sh, miss = X.shares(want[2])
    assert sh["triangle"] >= 0.15 and sh["medium"] >= 0.01 and sh["moving_sphere"] >= 0.01 and miss <= 0.6, (want[2], miss)
    got = _render(s, cam, W, H, spp, "auto")
    # (the top level — 7 records, 9 nodes — is staged; the pool and the bottom level are read from global memory)
    _assert_path(got, "bvh", 1, ALL_LDS)
    _assert_image(got, want, "field")


# ---- 5. reference scenes with a reachable mesh ------------------------------------------
PRESET_MESHES = {  # (centre, radius) of the glass and of the smooth metal icosphere(2)
    7: (((170.0, 330.0, 120.0), 90.0), ((400.0, 380.0, 180.0), 90.0)),
    8: (((330.0, 330.0, 60.0), 70.0), ((160.0, 230.0, 40.0), 70.0)),
}


def _preset_with_meshes(which, W, H):
    earth = nw.load_image(os.path.join(GOLD, "earthmap.jpeg"))
    s, cam = nw.preset(which, image=earth, aspect=W / H)
    (cg, rg), (cm, rm) = PRESET_MESHES[which]
    v, f = M.icosphere(2, rg, cg)
    s.add(s.mesh(v, f, mat=s.dielectric(1.5)))
    v, f = M.icosphere(2, rm, cm)
    s.add(s.mesh(v, f, normals=S.sphere_normals(v, cm, rm), smooth=True, mat=s.metal(s.solid(0.8, 0.85, 0.9), 0.05)))
    return s, cam


@pytest.mark.parametrize("accel", ["bvh", "grid"])
@pytest.mark.parametrize("which", [7, 8])
def test_reference_scenes_with_reachable_meshes_equal_the_oracle(which, accel):
    """cornell_smoke (7) and the final scene (8) with a glass icosphere(2) and
    a smooth metal one in view.  Oracle at (29, 23, 3): triangles win .208 (7)
    and .113 (8) of the hitting segments (at least 3% asked).  Both scenes have
    a grid the persistent kernel stages; on the BVH cornell_smoke's nodes and
    objects fit the LDS of two blocks per CU, the final scene's nodes alone."""
    W, H, spp = SMALL
    s, cam = _preset_with_meshes(which, W, H)
    want = X.oracle_image(("preset", which), s, cam, W, H, spp)
    sh, _ = X.shares(want[2])
    assert sh["triangle"] >= 0.03 and want[2]["medium"] > 0, sh
    got = _render(s, cam, W, H, spp, accel)
    _assert_path(got, accel, 1, GRID if accel == "grid" else ALL_LDS if which == 7 else NODES)
    _assert_image(got, want, f"preset {which} {accel}")


# ---- 6. edges -----------------------------------------------------------------------------
@pytest.mark.parametrize("edge", ["max_depth_1", "pinhole", "inside_glass", "seed_max"])
@pytest.mark.parametrize("shared", [False, True])
def test_mixed_scene_edges_equal_the_oracle(shared, edge):
    """max_depth = 1 (camera segments only), a pinhole camera, a camera inside
    the dielectric quarter's closed mesh, and seed 2**64 - 1, flattened with
    attributes (TRI = 2, BVH) and shared (TRI = 3).  Oracle's shares of the
    hitting segments (triangle, moving sphere, rectangle, box, medium) and of
    misses: max_depth_1 .228 .083 .289 .058 .063, 0 (every camera ray hits);
    pinhole .183 .098 .296 .079 .045, .222; seed_max .194 .093 .289 .073 .045,
    .223; inside_glass (looking through the glass at the media) .350 .041 .080
    .214 .041, .210."""
    W, H, spp = SMALL
    s = X.mixed_scene(shared, True)
    depth, seed = (1 if edge == "max_depth_1" else 50), (2 ** 64 - 1 if edge == "seed_max" else SEED)
    cam = X.inside_camera(W, H) if edge == "inside_glass" else X.mixed_camera(W, H, aperture=0.0 if edge == "pinhole" else 0.15)
    want = X.oracle_image(("edge", shared, edge), s, cam, W, H, spp, depth=depth, seed=seed)
    X.assert_mixed_conditions(want[2])
    if edge == "inside_glass":  # every camera ray starts inside the closed surface: it hits, and goes on
        assert want[1] >= 2 * W * H * spp, want[1]
    if edge == "max_depth_1":
        assert want[1] == W * H * spp
    got = _render(s, cam, W, H, spp, "auto" if shared else "bvh", depth, seed)
    _assert_path(got, "bvh", 1, ALL_LDS if shared else NODES)
    _assert_image(got, want, f"{edge} shared {shared}")


# ---- 7. hits and records with every kind present ---------------------------------------------
@pytest.fixture(scope="module")
def all_kind_rays():
    g = np.random.default_rng(77)
    rays = M.signed_zero_rays(g, 60_000, (-6.0, -2.0, -4.5), (10.0, 4.0, 8.5))  # (the last column: times in [0, 1))
    keys = g.integers(0, 2 ** 64, 60_000, dtype=np.uint64)
    return rays, keys


@pytest.mark.parametrize("walk", ["grid", "bvh", "shared"])
def test_hits_and_records_with_every_kind_present(walk, all_kind_rays):
    """60 000 rays with signed zeros, random times and random 64-bit medium
    keys over the mixed scene's bounds: debug_hits (index, t, box face) and
    debug_records (p, n, u, v, material) through the grid, the BVH and the
    two-level walk == the oracle, bitwise — box faces, medium keys and moving
    spheres' times under the triangle kernels.  Oracle: .709 of the rays hit, a
    box face wins .040, a medium .019, a moving sphere .038, a triangle .085."""
    rays, keys = all_kind_rays
    s = X.mixed_scene(walk == "shared", True)
    flat, fa = s.flat(), s.flat_attr()
    wi, wt, wface = O.nw_hits(flat, rays, keys, flat_attr=fa)
    ri, rt, wrec, wmat = O.nw_records(flat, rays, keys, flat_attr=fa)
    assert np.array_equal(ri, wi) and np.array_equal(rt[wi >= 0].view(np.int32), wt[wi >= 0].view(np.int32))
    kinds = np.where(wi >= 0, flat["obj"].reshape(-1, 16)[np.maximum(wi, 0), 12].view(np.int32), -1)
    share = {k: float((kinds == k).mean()) for k in range(8)}
    print(f"hit {(wi >= 0).mean():.3f} box face {(wface != -1).mean():.3f} by kind {share}")
    assert (wi >= 0).mean() >= 0.20 and (wface != -1).mean() >= 0.01, ((wi >= 0).mean(), (wface != -1).mean())
    assert (wface[kinds == 5] >= 0).all() and (wface[kinds != 5] == -1).all() and len(np.unique(wface)) == 7
    assert all(share[k] >= 0.01 for k in (1, 5, 6, 7)) and min(share[2], share[3], share[4]) > 0, share
    r = nw.NwRenderer(s)
    try:
        r.set_accel("auto" if walk == "shared" else walk)
        # (debug_hits and debug_records do not render: last_kernel() and last_staging() say nothing about them;
        # they walk what accel_info() names)
        info = r.accel_info()
        assert info["accel"] == ("bvh" if walk == "shared" else walk)
        assert (info["dims"] != (0, 0, 0)) == (walk != "shared"), info  # the grid was built (a scene with placements has none)
        assert (s.instancing_stats()["placements"] > 0) == (walk == "shared")
        gi, gt, gface = r.debug_hits(rays, keys)
        qi, qt, grec, gmat = r.debug_records(rays, keys)
    finally:
        r.close()
    want = np.column_stack([wi, wt.view(np.int32), wface])
    got = np.column_stack([gi, gt.view(np.int32), gface])
    for c, name in enumerate(("index", "t", "face")):
        bad = np.nonzero(got[:, c] != want[:, c])[0]
        assert bad.size == 0, f"{walk} hits {name}: {bad.size} rays differ, first {bad[:5]}: {got[bad[:5], c]} vs {want[bad[:5], c]}"
    want = np.column_stack([wi, rt.view(np.int32), wrec.view(np.int32), wmat])
    got = np.column_stack([qi, qt.view(np.int32), grec.view(np.int32), gmat])
    for c, name in enumerate(("index", "t", "px", "py", "pz", "nx", "ny", "nz", "u", "v", "material")):
        bad = np.nonzero(got[:, c] != want[:, c])[0]
        assert bad.size == 0, (f"{walk} records {name}: {bad.size} rays differ, first {bad[:5]} kinds {kinds[bad[:5]]}: "
                               f"{got[bad[:5], c]} vs {want[bad[:5], c]}")
