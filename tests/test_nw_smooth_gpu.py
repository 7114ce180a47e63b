"""Triangle attributes of the Next-Week renderer on the GPU: the gfx950
kernels' hit record with interpolated normals and texture coordinates
(make_rec's attribute path, through rt_nw_debug_records and
rt_nw_debug_trace) against the plain C++ restatement
(tests/native/nw_smooth_ref.cpp, itself checked on the CPU by
tests/test_nw_smooth.py) bit for bit — through the uniform grid and the BVH,
from LDS and from global memory, whole paths — the image invariants (grid ==
BVH, chunk splits, strips, persistent == one-shot), that a mesh built with
flags 0 renders as before, that uvs reach the image texture, and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd.nextweek as nw
import nw_mesh_util as M
import nw_smooth_util as S

pytestmark = pytest.mark.gpu
SEED = 1984
NAMES = ("index", "t", "px", "py", "pz", "nx", "ny", "nz", "u", "v", "material")


def world_grazing_rays(subdiv, instance):
    """S.grazing_rays of the local mesh, carried into the world of
    smooth_scene(instance=True): world = R local + offset."""
    v, f = S.icosphere(subdiv)
    g = S.grazing_rays(v, f)
    if instance:
        th = np.radians(30.0)
        R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        o = g[:, :3].astype(np.float64) @ R.T + np.array([0.4, 0.3, -0.5])
        g = np.column_stack([o, g[:, 3:6].astype(np.float64) @ R.T, g[:, 6]]).astype(np.float32)
    return g


def assert_records_equal(s, rays, accels, min_hit=0.2, graze=None, graze_counts=True):
    """debug_records of every ray equals the checker's record bit for bit:
    index, t, p, n, u, v, material.  graze: rays (appended) of which, on the
    320-triangle mesh (graze_counts), at least 500 must take the side rule's
    fallback and 10 000 the smooth normal."""
    a = S.scene_arrays(s)
    allr = rays if graze is None else np.concatenate([rays, graze])
    wi, wt, wrec, wmat, side = S.ref_records(a, allr)
    assert (wi[:len(rays)] >= 0).mean() >= min_hit, (wi[:len(rays)] >= 0).mean()
    if graze is not None:
        gs = side[len(rays):]
        print(f"grazing rays: {(gs == S.SIDE_FALLBACK).sum()} fallbacks, {(gs == S.SIDE_SMOOTH).sum()} smooth")
        assert (gs == S.SIDE_FALLBACK).sum() >= (500 if graze_counts else 1) and (gs == S.SIDE_SMOOTH).sum() >= 10_000
    want = np.column_stack([wi, wt.view(np.int32), wrec.view(np.int32), wmat])
    r = nw.NwRenderer(s)
    try:
        for accel in accels:
            r.set_accel(accel)
            assert r.accel_info()["accel"] == accel
            gi, gt, grec, gmat = r.debug_records(allr)
            got = np.column_stack([gi, gt.view(np.int32), grec.view(np.int32), gmat])
            for c, name in enumerate(NAMES):
                bad = np.nonzero(got[:, c] != want[:, c])[0]
                assert bad.size == 0, (f"{accel} {name}: {bad.size} rays differ, first {bad[:5]} side {side[bad[:5]]}: "
                                       f"{got[bad[:5], c]} vs {want[bad[:5], c]}")
            hi, ht, _ = r.debug_hits(allr)  # the walk is the one debug_hits reports
            assert np.array_equal(hi, gi) and np.array_equal(ht[gi >= 0].view(np.int32), gt[gi >= 0].view(np.int32))
    finally:
        r.close()
    return a, wi, side


# ---- records, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("instance", [False, True])
def test_records_small_mesh_and_spheres_grid_then_bvh(instance):
    """320 smooth + uv triangles in four materials (one image-textured) + 5
    spheres, 50 000 rays and the 20 000 grazing ones, through the grid (staged
    in LDS) and the BVH; once with the mesh under rotate_y(30) + translate."""
    s = S.smooth_scene(instance=instance)
    a, idx, side = assert_records_equal(s, S.hit_rays(s.flat(), 50_000, 41 + instance), ["grid", "bvh"],
                                        graze=world_grazing_rays(2, instance))
    kinds = a["obj"][idx[idx >= 0], 12].view(np.int32)
    assert (kinds == 7).sum() > 10_000 and (kinds == 0).sum() > 2_000  # both kinds win
    mats = a["obj"][idx[(idx >= 0) & (idx < 320)], 13].view(np.int32)
    assert len(np.unique(mats)) == 4  # every material's quarter is hit


def test_records_large_mesh_from_global_memory():
    """5 120 triangles: the BVH's nodes and the objects are walked from global
    memory (the one-shot kernel; rt_nw_ctx_last_staging of a small render).
    The grazing rays go along; on this finer mesh ng and ns are 4 x closer, so
    fewer of them take the fallback (269 by the checker) than the 500 asked of
    the 320-triangle mesh."""
    s = S.smooth_scene(4, spheres=False)
    assert s.flat()["n_obj"] == 5120 and len(s.flat_attr()["attr"]) == 5120
    assert_records_equal(s, S.hit_rays(s.flat(), 30_000, 44), ["bvh"], graze=world_grazing_rays(4, False),
                         graze_counts=False)
    r = nw.NwRenderer(s)
    try:
        r.set_accel("bvh")
        img = r.render(nw.camera((6, 2.5, 7), M.CENTRE, (0, 1, 0), 35, 1.5, 0.0, 9.0), 24, 16, 2, 50, SEED)
        assert r.last_staging() == {"nodes_lds": False, "objects_lds": False} and r.last_kernel()["persistent"] == 0
        assert np.isfinite(img).all() and img.std() > 0
    finally:
        r.close()


def test_records_flat_and_attributed_triangles_in_one_group():
    """One group of a smooth + uv part, a flat part (flags 0), a uv-only part
    and a smooth-only part, all under the image texture."""
    s = S.smooth_scene(mixed_flat=True)
    a, idx, side = assert_records_equal(s, S.hit_rays(s.flat(), 30_000, 45), ["grid", "bvh"])
    tri = idx[(idx >= 0) & (idx < 320)]
    assert all(((tri // 80) == part).sum() > 500 for part in range(4))
    assert (side[(idx >= 80) & (idx < 240)] == S.SIDE_NONE).all()


# ---- whole paths ----------------------------------------------------------------------
def test_traced_paths_equal_reference_segment_by_segment():
    """200 (pixel, sample) traces at depth 50 through spheres and smooth
    lambertian, metal, glass and image-emitting triangles: every segment's
    winner, t and record normal — and the next segment's origin, the record's
    point — are the checker's for that segment's (o, d), bit for bit."""
    W, H = 48, 32
    s = S.smooth_scene(mats="light", ground=True)
    a = S.scene_arrays(s)
    kinds = a["obj"][:, 12].view(np.int32)
    cam = nw.camera((6, 2.5, 7), M.CENTRE, (0, 1, 0), 35, W / H, 0.0, 9.0)
    g = np.random.default_rng(9)
    r = nw.NwRenderer(s)
    longest, ends_on_triangle, nseg, smooth_segments = 0, 0, 0, 0
    try:
        for _ in range(200):
            i, j, smp = int(g.integers(8, W - 8)), int(g.integers(6, H - 4)), int(g.integers(0, 64))
            seg, ids = r.debug_trace(cam, W, H, i, j, smp, max_depth=50, seed=SEED, cap=64)
            assert len(seg) >= 1
            wi, wt, wrec, _, side = S.ref_records(a, seg[:, :6])
            assert np.array_equal(ids[:, 0], wi), (i, j, smp, ids[:, 0], wi)
            hit = wi >= 0
            assert np.array_equal(seg[hit, 6].view(np.int32), wt[hit].view(np.int32)), (i, j, smp)
            assert np.array_equal(seg[hit, 7:10].view(np.int32), wrec[hit, 3:6].view(np.int32)), (i, j, smp, side)
            # the next segment starts at the record's point
            assert np.array_equal(seg[1:, :3].view(np.int32), wrec[:len(seg) - 1, :3].view(np.int32)), (i, j, smp)
            longest = max(longest, len(seg))
            nseg += len(seg)
            smooth_segments += int((side == S.SIDE_SMOOTH).sum())
            ends_on_triangle += int(ids[-1, 0] >= 0 and kinds[ids[-1, 0]] == 7)
    finally:
        r.close()
    # as the flat mesh's trace test asks: long paths and triangles are reached — here, with a smooth normal too
    assert longest >= 3 and ends_on_triangle >= 1 and smooth_segments >= 1, (longest, ends_on_triangle, nseg, smooth_segments)


# ---- image invariants -------------------------------------------------------------------
W10, H10, SPP10 = 64, 40, 70


def _render(scene, accel="bvh", env=None, monkeypatch=None, rows=None):
    for k, val in (env or {}).items():
        monkeypatch.setenv(k, val)  # read when the context is created
    cam = nw.camera((6, 2.5, 7), M.CENTRE, (0, 1, 0), 35, W10 / H10, 0.0, 9.0)
    r = nw.NwRenderer(scene)
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


def _render_a(*args, **kw):
    return _render(S.smooth_scene(ground=True), *args, **kw)


@pytest.fixture(scope="module")
def base_image():
    img, k = _render_a("bvh")
    assert k["persistent"] == 1 and np.isfinite(img).all()
    return img


def test_image_differs_from_the_flat_mesh(base_image):
    """The attributes are in use: the same mesh flat renders another image."""
    flat_img, _ = _render(_flat_twin(), "bvh")
    assert not np.array_equal(flat_img, base_image)


def _flat_twin(attr_call=False):
    """smooth_scene(ground=True) with the mesh built flat: by rt_nw_mesh, or by
    rt_nw_mesh_attr with flags 0."""
    s = nw.Scene()
    grey = s.lambertian(s.solid(0.6, 0.5, 0.4))
    v, f = S.icosphere(2)
    nrm = np.ascontiguousarray(S.sphere_normals(v))
    ms = [grey, s.metal(s.solid(0.8, 0.8, 0.9), 0.3), s.dielectric(1.5), s.lambertian(s.image(S.TEXTURE))]
    parts = []
    for k in range(4):
        fk = np.ascontiguousarray(f[k * 80:(k + 1) * 80], np.int32)
        parts.append(s.mesh_attr(np.ascontiguousarray(v), fk, nrm, None, None, None, 0, ms[k]) if attr_call
                     else s.mesh(v, fk, normals=nrm, mat=ms[k]))
    s.add(s.group(parts))
    sm = [grey, s.metal(s.solid(0.7, 0.6, 0.5), 0.0), s.dielectric(1.5), grey, s.lambertian(s.solid(0.9, 0.2, 0.2))]
    for (c, r), m in zip(S.SPHERES, sm):
        s.add(s.sphere(c, r, m))
    s.add(s.sphere((0, -1002, 0), 1000, s.lambertian(s.checker(s.solid(0.2, 0.3, 0.1), s.solid(0.9, 0.9, 0.9)))))
    s.set_background(0.7, 0.8, 1.0)
    return s


def test_image_grid_equals_bvh(base_image):
    img, k = _render_a("grid")
    assert k["grid"] == 1 and np.array_equal(img, base_image)


@pytest.mark.parametrize("accel", ["bvh", "grid"])
def test_image_chunk_splits(accel, base_image, monkeypatch):
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


# ---- flat is untouched ----------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["bvh", "grid"])
def test_flags_zero_renders_as_rt_nw_mesh(accel):
    a, _ = _render(_flat_twin(False), accel)
    b, _ = _render(_flat_twin(True), accel)
    assert np.array_equal(a, b) and a.std() > 0


# ---- uvs reach the texture -----------------------------------------------------------------
def test_uvs_reach_the_image_texture():
    """An emitting unit quad of two triangles under a 4 x 4 image of sixteen
    colours with uv = (y, 1 - x), a quarter turn against position, seen head-on
    (no aperture, depth 1): a pixel whose footprint lies inside one texel
    holds exactly spp x that texel's colour.  The view spans 1.1 units over 40
    pixels (0.0275 per pixel, 9.09 pixels per texel), so about (8 / 9.09)^2 =
    77% of the quad's pixels lie inside one texel."""
    W = H = 40
    spp, span, D = 4, 1.1, 2.0
    img = (np.arange(48, dtype=np.uint8).reshape(4, 4, 3) * 5 + 7).astype(np.uint8)
    assert len(np.unique(img.reshape(-1, 3), axis=0)) == 16
    s = nw.Scene()
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float64)
    uv = np.column_stack([v[:, 1], 1 - v[:, 0]])
    s.add(s.mesh(v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), uvs=uv, mat=s.diffuse_light(s.image(img))))
    s.set_background(0, 0, 0)
    cam = nw.camera((0.5, 0.5, D), (0.5, 0.5, 0), (0, 1, 0), np.degrees(2 * np.arctan(span / (2 * D))), 1.0, 0.0, D)
    r = nw.NwRenderer(s)
    try:
        got = r.render(cam, W, H, spp, 1, SEED)
    finally:
        r.close()
    edge = 0.5 + (np.arange(W + 1) / W - 0.5) * span  # pixel i covers x in [edge[i], edge[i + 1]]; rows alike in y
    margin = 1e-4
    lo, hi = edge[:-1] - margin, edge[1:] + margin
    inside = (lo > 0) & (hi < 1)
    cell = np.where(np.floor(lo * 4) == np.floor(hi * 4), np.floor(lo * 4), -1).astype(int)
    one, f255 = np.float32(1), np.float32(255)
    quad_pixels = checked = 0
    for j in range(H):
        for i in range(W):
            if not (inside[i] and inside[j]):
                continue
            quad_pixels += 1
            if cell[i] < 0 or cell[j] < 0:
                continue
            # image_texture::value: u = y picks the column (+ the shift), 1 - v = x the row from the top
            ti, tj = (cell[j] + 4 // 2 + 4 // 3) % 4, cell[i]
            c = (one / f255) * img[tj, ti].astype(np.float32)
            want = (spp * c.astype(np.float64)).astype(np.float32)
            assert np.array_equal(got[j, i], want), (i, j, got[j, i], want)
            checked += 1
    assert quad_pixels > 1000 and checked >= 0.6 * quad_pixels, (checked, quad_pixels)
    assert (got[0] == 0).all() and (got[:, 0] == 0).all()  # the border sees the background


# ---- the CLI -------------------------------------------------------------------------------
def _sphere_obj():
    v, f = S.icosphere(1)
    n = S.sphere_normals(v)
    lines = ["v %r %r %r" % tuple(float(x) for x in p) for p in v]
    lines += ["vn %r %r %r" % tuple(float(x) for x in p) for p in n]
    lines += ["vt %r %r" % (float(0.5 + 0.5 * p[0]), float(0.5 + 0.5 * p[1])) for p in n]
    lines += ["f " + " ".join(f"{c + 1}/{c + 1}/{c + 1}" for c in t) for t in f]
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("mat", ["lambertian", "metal"])
def test_cli_obj_smooth_texture_matches_library(tmp_path, mat):
    exe = os.path.join(os.path.dirname(nw.__file__), "bin", "rtmi_nw_render")
    path, ppm, out = tmp_path / "ball.obj", tmp_path / "tex.ppm", tmp_path / "o.ppm"
    path.write_text(_sphere_obj())
    tex = np.random.default_rng(3).integers(0, 256, (8, 8, 3)).astype(np.uint8)
    ppm.write_bytes(b"P6\n8 8\n255\n" + tex.tobytes())
    W, H, spp = 24, 16, 4
    subprocess.run([exe, "--obj", str(path), "--obj-mat", mat, "--obj-smooth", "--obj-texture", str(ppm), "--width", str(W),
                    "--height", str(H), "--spp", str(spp), "--out", str(out)], check=True, capture_output=True, timeout=120)
    tok = out.read_text().split()
    assert tok[:4] == ["P3", str(W), str(H), "255"]
    got = np.array(tok[4:], np.int64).reshape(H, W, 3)
    s, cam, n = nw.obj_stage(path, mat, aspect=W / H, smooth=True, texture=tex)
    assert n == 80 and (s.flat_attr()["attr"][:, 15].view(np.int32) == 3).all()
    r = nw.NwRenderer(s)
    sums = r.render(cam, W, H, spp, 50, SEED)
    r.close()
    mean = (sums / np.float32(spp)).astype(np.float32)
    want = np.floor(255.99 * np.sqrt(mean).astype(np.float32).astype(np.float64)).astype(np.int64)[::-1]
    assert np.array_equal(got, want)
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 20  # a picture, not a flat colour
    s0, _, _ = nw.obj_stage(path, mat, aspect=W / H)  # the flags reached the render
    r = nw.NwRenderer(s0)
    flat_sums = r.render(cam, W, H, spp, 50, SEED)
    r.close()
    assert not np.array_equal(flat_sums, sums)
    for extra in (["--obj-smooth"], ["--obj-gen-normals"], ["--obj-texture", str(ppm)]):
        p = subprocess.run([exe, "--scene", "2"] + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "--obj" in p.stderr
