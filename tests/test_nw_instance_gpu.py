"""Shared meshes (Scene.shared) on the GPU: the two-level walk of the gfx950
kernels against today's path — a second context holding the same scene built
WITHOUT shared, its flattened copies under the one-level BVH — bit for bit:
closest hits, hit records, whole images in every kernel shape, bottom levels
far beyond LDS, watertightness, and the CLI's --obj-copies."""
import os
import subprocess

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd.nextweek as nw
import nw_instance_util as U
import nw_mesh_util as M
import nw_smooth_util as SU

pytestmark = pytest.mark.gpu
SEED = 1984


def _both(build):
    """(renderer of the shared build, renderer of the flattened build on the BVH)."""
    a, b = nw.NwRenderer(build(True)), nw.NwRenderer(build(False))
    b.set_accel("bvh")
    assert a.accel_info()["accel"] == "bvh" and b.accel_info()["accel"] == "bvh"
    return a, b


def _assert_same_hits(a, b, rays):
    gi, gt, gf = a.debug_hits(rays)
    wi, wt, wf = b.debug_hits(rays)
    for name, x, y in (("index", gi, wi), ("t", gt.view(np.int32), wt.view(np.int32)), ("face", gf, wf)):
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, f"{name}: {bad.size} rays differ, first {bad[:5]}: {x[bad[:5]]} vs {y[bad[:5]]}"
    return wi, wt


# ---- 1. closest hits ---------------------------------------------------------
def test_hits_equal_the_flattened_copies():
    flat = U.five_placements(False).flat()
    rays = SU.hit_rays(flat, 100_000, 41)
    # the conditions, from the reference side alone (the CPU checker on the flat view)
    want_i, want_t = M.ref_closest(flat, rays)
    first = [320 * p for p in range(5)]
    pl = U.placement_of(want_i, first, 320)
    assert (pl >= 0).mean() >= 0.20, (pl >= 0).mean()
    for p in range(4):
        assert (pl == p).mean() >= 0.01, (p, (pl == p).mean())
    # the fifth placement coincides with the fourth: wherever the fourth wins, the fifth's copy of the
    # same triangle hits at the same t (the flat view without the fourth's rows says so) and loses the tie
    obj, _ = M.flat_arrays(flat)
    less = dict(flat, obj=np.concatenate([obj[:960], obj[1280:]]).reshape(-1))
    li, lt = M.ref_closest(less, rays)
    tie = pl == 3
    assert tie.sum() >= 1000 and (pl == 4).sum() == 0
    assert np.array_equal(li[tie], want_i[tie]) and np.array_equal(lt[tie].view(np.int32), want_t[tie].view(np.int32))
    a, b = _both(U.five_placements)
    try:
        gi, gt = _assert_same_hits(a, b, rays)
        assert np.array_equal(gi, want_i) and np.array_equal(gt.view(np.int32), want_t.view(np.int32))
        st = U.five_placements(True).instancing_stats()
        assert a.info() == (st["top_leaves"], st["top_nodes"]) and st["top_leaves"] == 5 + len(U.SPHERES)  # the top level's counts
    finally:
        a.close()
        b.close()


# ---- 2. hit records ----------------------------------------------------------
ROT2, OFF2 = 40.0, (1.5, -0.4, 2.2)


def _smooth_placed(shared):
    s = nw.Scene()
    v, f = M.icosphere(2)
    mesh = s.mesh(v, f, normals=SU.sphere_normals(v), uvs=SU.affine_uvs(v), smooth=True, mat=s.lambertian(s.image(SU.TEXTURE)))
    h = s.shared(mesh) if shared else mesh
    s.add(s.translate(s.rotate_y(h, ROT2), OFF2))
    s.add(s.sphere((0, -1002, 0), 1000, s.lambertian(s.solid(0.5, 0.5, 0.5))))
    s.set_background(0.7, 0.8, 1.0)
    return s


def _to_world(rays, rot, off):
    """Local rays (rows o.xyz d.xyz ...) through rotate_y(rot) then translate(off), float32."""
    th = np.radians(rot)
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])  # local -> world
    out = np.array(rays, np.float32)
    out[:, :3] = (rays[:, :3].astype(np.float64) @ R.T + np.asarray(off, np.float64)).astype(np.float32)
    out[:, 3:6] = (rays[:, 3:6].astype(np.float64) @ R.T).astype(np.float32)
    return out


def test_records_equal_the_flattened_copies():
    v, f = M.icosphere(2)
    local = np.concatenate([M.signed_zero_rays(np.random.default_rng(5), 10_000, np.array(M.CENTRE) - 2.6, np.array(M.CENTRE) + 2.6),
                            SU.grazing_rays(v, f, 10_000)])
    rays = _to_world(local, ROT2, OFF2)
    a, b = _both(_smooth_placed)
    try:
        gi, gt, grec, gmat = a.debug_records(rays)
        wi, wt, wrec, wmat = b.debug_records(rays)
    finally:
        a.close()
        b.close()
    on_mesh = (wi >= 0) & (wi < 320)
    assert on_mesh.mean() > 0.3 and on_mesh[10_000:].mean() > 0.5, (on_mesh.mean(), on_mesh[10_000:].mean())
    assert (wrec[on_mesh][:, 6:8] != 0).any()  # the texture reads u, v
    assert np.array_equal(gi, wi) and np.array_equal(gt.view(np.int32), wt.view(np.int32)) and np.array_equal(gmat, wmat)
    bad = np.nonzero((grec.view(np.int32) != wrec.view(np.int32)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:5], grec[bad[:3]], wrec[bad[:3]])


# ---- 3. images ---------------------------------------------------------------
CAM3 = dict(lookfrom=(7, 3.0, 9), lookat=(0.3, 0.2, 0.9), vfov=35)
_REF3 = {}


def _cam3(W, H):
    return nw.camera(CAM3["lookfrom"], CAM3["lookat"], (0, 1, 0), CAM3["vfov"], W / H, 0.0, 10.0)


def _reference3(mats, W, H):
    """The flattened build's image and segment count (rendered once per case)."""
    key = (mats, W, H)
    if key not in _REF3:
        r = nw.NwRenderer(U.mixed_placements(False, mats))
        try:
            r.set_accel("bvh")
            img = r.render(_cam3(W, H), W, H, 16, 10, SEED)
            _REF3[key] = (img, r.last_segments())
        finally:
            r.close()
        assert np.isfinite(img).all() and img.std() > 0
    return _REF3[key]


@pytest.mark.parametrize("mats,W,H,persist", [("mixed", 64, 48, "1"), ("mixed", 64, 48, "0"), ("light", 64, 48, "1"),
                                              ("mixed", 61, 45, "1"), ("mixed", 61, 45, "0")])
def test_images_equal_the_flattened_copies(mats, W, H, persist, monkeypatch):
    want, want_segs = _reference3(mats, W, H)
    monkeypatch.setenv("RTMI_NW_PERSIST", persist)  # read when the context is created
    r = nw.NwRenderer(U.mixed_placements(True, mats))
    try:
        got = r.render(_cam3(W, H), W, H, 16, 10, SEED)
        k, st = r.last_kernel(), r.last_staging()
        assert k["persistent"] == int(persist) and k["grid"] == 0 and st == {"nodes_lds": True, "objects_lds": True}, (k, st)
        assert r.last_segments() == want_segs
        assert np.array_equal(got, want), f"max |d| {np.abs(got - want).max()}"
    finally:
        r.close()


def test_image_row_strips_equal_the_flattened_copies():
    import torch

    W, H = 64, 48
    want, _ = _reference3("mixed", W, H)
    r = nw.NwRenderer(U.mixed_placements(True))
    try:
        strip = torch.full((17, W, 3), -1.0, dtype=torch.float32, device="cuda")
        st = torch.cuda.Stream()
        r.render_rows(_cam3(W, H), W, H, 16, 10, SEED, 1, 3, 17, strip.data_ptr(), st.cuda_stream)  # rows 1, 4, ..., 46; one past H
        st.synchronize()
        img = strip.cpu().numpy()
    finally:
        r.close()
    assert np.array_equal(img[:16], want[1::3]) and (img[16] == 0).all()


def test_traces_equal_the_flattened_copies():
    W, H = 64, 48
    a, b = _both(U.mixed_placements)
    g = np.random.default_rng(12)
    try:
        nseg, on_mesh = 0, 0
        for _ in range(40):
            i, j, smp = int(g.integers(4, W - 4)), int(g.integers(4, H - 4)), int(g.integers(0, 16))
            sa, ia = a.debug_trace(_cam3(W, H), W, H, i, j, smp, max_depth=10, seed=SEED)
            sb, ib = b.debug_trace(_cam3(W, H), W, H, i, j, smp, max_depth=10, seed=SEED)
            assert np.array_equal(ia, ib) and np.array_equal(sa.view(np.int32), sb.view(np.int32)), (i, j, smp)
            nseg += len(sa)
            on_mesh += int(((ib[:, 0] >= 0) & (ib[:, 0] < 960)).sum())
    finally:
        a.close()
        b.close()
    assert nseg > 60 and on_mesh > 20, (nseg, on_mesh)


# ---- 4. bottom levels beyond LDS ----------------------------------------------
@pytest.mark.parametrize("subdiv,n,ntri", [(4, 3, 5120), (5, 16, 20480)])
def test_hits_large_shared_meshes(subdiv, n, ntri):
    shared, plain = U.field(True, subdiv, n), U.field(False, subdiv, n)
    st = shared.instancing_stats()
    assert (st["meshes"], st["placements"], st["pool_triangles"], st["top_leaves"]) == (1, n, ntri, n)
    assert st["bottom_nodes"] * 32 > 160 * 1024 * (subdiv == 5)  # (5: the bottom level alone exceeds a CU's LDS)
    flat = plain.flat()
    assert flat["n_obj"] == n * ntri
    side = int(np.ceil(np.sqrt(n)))  # U.field: copies 4 apart, each turned about the y axis
    lo, hi = np.array([-3.0, -2.5, -3.0]), np.array([4.0 * (side - 1) + 3.0, 2.5, 4.0 * (side - 1) + 3.0])
    rays = M.signed_zero_rays(np.random.default_rng(50 + subdiv), 20_000, lo, hi)
    a, b = nw.NwRenderer(shared), nw.NwRenderer(plain)
    try:
        b.set_accel("bvh")
        wi, _ = _assert_same_hits(a, b, rays)
    finally:
        a.close()
        b.close()
    pl = wi[wi >= 0] // ntri
    assert (wi >= 0).mean() > 0.1 and len(np.unique(pl)) == n, ((wi >= 0).mean(), np.unique(pl))


# ---- 5. watertight ---------------------------------------------------------------
def test_placed_mesh_is_watertight():
    v, f = M.icosphere(2)

    def build(shared):
        s = nw.Scene()
        mesh = s.mesh(v, f, mat=s.lambertian(s.solid(0.5, 0.5, 0.5)))
        s.add(s.translate(s.rotate_y(s.shared(mesh) if shared else mesh, 75.0), (-2.9, 0.3, 0.8)))
        return s

    local = np.zeros((150_000 + 2 * 162 + 480 + 6, 7), np.float32)
    local[:, :6] = M.watertight_rays(v, f)
    rays = _to_world(local, 75.0, (-2.9, 0.3, 0.8))
    a, b = _both(build)
    try:
        wi, _ = _assert_same_hits(a, b, rays)
    finally:
        a.close()
        b.close()
    assert (wi < 0).sum() == 0, np.nonzero(wi < 0)[0][:10]


# ---- 6. the CLI ------------------------------------------------------------------
def _run_cli(exe, path, out, extra, W=48, H=32, spp=4):
    subprocess.run([exe, "--obj", str(path), "--width", str(W), "--height", str(H), "--spp", str(spp), "--out", str(out), *extra],
                   check=True, capture_output=True, timeout=120)
    tok = out.read_text().split()
    assert tok[:4] == ["P3", str(W), str(H), "255"]
    return np.array(tok[4:], np.int64).reshape(H, W, 3)


def test_cli_obj_copies_matches_library(tmp_path):
    exe = os.path.join(os.path.dirname(nw.__file__), "bin", "rtmi_nw_render")
    path = tmp_path / "cube.obj"
    path.write_text(M.cube_obj("a//n", quads=True, scale=3.0, offset=(5.0, -2.0, 1.0)))
    W, H, spp = 48, 32, 4
    got = _run_cli(exe, path, tmp_path / "c3.ppm", ["--obj-copies", "3"])
    s, cam, n = nw.obj_stage(path, aspect=W / H, copies=3)
    assert n == 12 and s.instancing_stats()["placements"] == 9
    r = nw.NwRenderer(s)
    sums = r.render(cam, W, H, spp, 50, SEED)
    r.close()
    mean = (sums / np.float32(spp)).astype(np.float32)
    want = np.floor(255.99 * np.sqrt(mean).astype(np.float32).astype(np.float64)).astype(np.int64)[::-1]
    assert np.array_equal(got, want)
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 20  # a picture, not a flat colour
    one = _run_cli(exe, path, tmp_path / "c1.ppm", ["--obj-copies", "1"])
    plain = _run_cli(exe, path, tmp_path / "c0.ppm", [])
    assert np.array_equal(one, plain) and not np.array_equal(one, got)
    p = subprocess.run([exe, "--scene", "2", "--obj-copies", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--obj-copies" in p.stderr
