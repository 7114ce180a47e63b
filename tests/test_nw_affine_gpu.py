"""Affine placements (Scene.transform) on the GPU: the TRI = 5 kernels.  The
flat view of an affine placement is baked, not a bit-for-bit expansion, so the
oracle alone cannot check these scenes: closest hits, records and every segment
of traced paths are compared bit for bit with the merged brute force of
tests/nw_affine_util.py (the checker of tests/native/nw_affine_ref.cpp over the
affine placements, the oracle over everything else); images are compared across
kernel shapes and against the hand-built frozen scene, and statistically against
a render of the baked flat view."""
import math
import os
import subprocess

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd.nextweek as nw
import nw_affine_util as AU
import nw_instance_util as U
import nw_mesh_util as M
import nw_motion_util as V
import nw_smooth_util as SU
from conftest import record_parity_stats

pytestmark = pytest.mark.gpu
SEED = 1984
THIRD = float(np.float32(1) / np.float32(3))
ALL_LDS = {"nodes_lds": True, "objects_lds": True}
bits = AU.bits


def _ctx(scene, tri=5):
    r = nw.NwRenderer(scene)
    assert r.scene_tri() == tri and r.accel_info()["accel"] == "bvh", (r.scene_tri(), tri)
    return r


def _cam(T0, T1, W, H):
    return nw.camera((2.0, 4.5, 15.0), (0.4, 0.4, 1.4), (0, 1, 0), 40, W / H, 0.0, 10.0, T0, T1)


@pytest.fixture(scope="module")
def scene_a():
    return AU.scene_a()


def _crowded(pl_or_T, side):
    """Scene A among side x side small spheres: top-level nodes (and records) too many for a block's LDS."""
    pl = AU.scene_a(T=pl_or_T)
    s = pl.scene
    m = s.lambertian(s.solid(0.3, 0.6, 0.8))
    for i in range(side):
        for k in range(side):
            s.add(s.sphere((-6 + 12 * i / (side - 1), -4.2 + 0.3 * ((i + k) % 3), -5 + 12 * k / (side - 1)), 0.12, m))
    return pl


# ---- 8. hits ---------------------------------------------------------------------------
@pytest.mark.parametrize("crowd", [0, 60])
def test_hits_equal_the_merged_brute_force(crowd):
    """Shares of the rays won by the three affine placements under the brute force, per time group (no crowd):
    0: .073 .107 .092   1: .090 .103 .097   0.5: .078 .101 .101   1/3: .083 .102 .089   0.1: .080 .102 .087
    0.25: .080 .103 .097   0.75: .076 .114 .096   nextafter(1, 0): .085 .099 .098   (crowd 60: .053 to .079)
    crowd: the top level in global memory for the render kernels too (debug_hits always walks it from there)."""
    pl = _crowded(None, crowd) if crowd else AU.scene_a()
    rays = AU.a_rays(pl, 40_000, 43, grazing=4_000)
    wi, wt, wf, wins = AU.merged(pl, rays)
    place = U.placement_of(wi, pl.first, pl.n_tri)
    for g, T in enumerate(V.RAY_TIMES):
        sel = np.arange(len(rays)) % 8 == g
        shares = [float((place[sel] == p).mean()) for p in pl.affine]
        print(f"T {T}: shares " + " ".join(f"{x:.3f}" for x in shares))
        assert min(shares) >= 0.05, (T, shares)
    assert (wf[wi >= 0] >= 0).any() and (place == 0).any() and (place == 4).any()  # the box, the classical placements
    a = _ctx(pl.scene)
    try:
        gi, gt, gf = a.debug_hits(rays)
    finally:
        a.close()
    for what, x, y in (("index", gi, wi), ("t", bits(gt), bits(wt)), ("face", gf, wf)):
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, (what, bad.size, bad[:5], x[bad[:5]], y[bad[:5]], rays[bad[:3]])


# ---- 9. records ------------------------------------------------------------------------
def test_records_equal_the_checker(scene_a):
    pl = scene_a
    rays = AU.a_rays(pl, 20_000, 5, grazing=10_000)
    wi, wt, wrec, wmat, wside, wins = AU.merged(pl, rays, records=True)
    on = wins.mean()
    fallback = (wside[wins] == SU.SIDE_FALLBACK).mean()
    print(f"on an affine placement {on:.3f}; of those the side rule fell back to the geometric normal {fallback:.3f}")
    assert on > 0.3 and fallback >= 0.01, (on, fallback)
    assert (wrec[wins][:, 6:8] != 0).any()  # the texture reads u, v
    a = _ctx(pl.scene)
    try:
        gi, gt, grec, gmat = a.debug_records(rays)
    finally:
        a.close()
    hit = wi >= 0
    assert np.array_equal(gi, wi) and np.array_equal(bits(gt)[hit], bits(wt)[hit]) and np.array_equal(gmat[hit], wmat[hit])
    bad = np.nonzero((bits(grec) != bits(wrec)).any(axis=1) & hit)[0]
    assert bad.size == 0, (bad.size, bad[:5], wins[bad[:5]], grec[bad[:3]], wrec[bad[:3]])


# ---- 10. a large mesh -------------------------------------------------------------------
def test_large_mesh_hits_equal_the_brute_force():
    v, f = M.icosphere(4)
    chains = [[("transform", nw.affine(scale=1.5, axis=(1, 1, 0), angle=40.0, translate=(-2.6, 0.5, -0.6)))],
              [("rotate_y", 20.0), ("transform", AU.shear(0.5, (2.0, 0.5, 1.0), (2.8, -1.0, 0.6)))],
              [("move", *AU.A_MOVE), ("transform", nw.affine(scale=(1.7, 1.2, 1.5), axis=(0, 1, 1), angle=25.0))]]
    pl = AU.placed(lambda s: s.mesh(v, f, mat=s.lambertian(s.solid(0.6, 0.5, 0.4))), chains, 5120)
    assert pl.scene.instancing_stats()["pool_triangles"] == 5120
    rays = AU.a_rays(pl, 20_000, 9)
    wi, wt, _, _ = AU.affine_closest(pl, rays)
    assert (wi >= 0).mean() > 0.15 and len(np.unique(wi)) > 3000
    a = _ctx(pl.scene)
    try:
        gi, gt, gf = a.debug_hits(rays)
    finally:
        a.close()
    hit = wi >= 0
    assert np.array_equal(gi, wi) and np.array_equal(bits(gt)[hit], bits(wt)[hit]) and (gf == -1).all()
    assert np.isinf(gt[~hit]).all()


# ---- 11. paths --------------------------------------------------------------------------
def test_open_shutter_segments_equal_the_merged_brute_force(scene_a):
    """64 pixels x 2 samples with the shutter open: every segment's ray (its o
    is the record's p of the segment before), t, winner and normal are the
    merged brute force's at that ray and the sample's time."""
    pl, W, H = scene_a, 48, 32
    g = np.random.default_rng(21)
    pix = [(int(g.integers(0, W)), int(g.integers(4, H))) for _ in range(64)]
    a = _ctx(pl.scene)
    rows, ids, starts, times = [], [], [], []
    try:
        for i, j in pix:
            for smp in (0, 1):
                seg, wid, t = a.debug_trace(_cam(0.0, 1.0, W, H), W, H, i, j, smp, max_depth=20, seed=SEED, with_time=True)
                assert 0.0 <= t <= 1.0 and len(seg) >= 1
                starts.append(len(rows))
                times.append(float(t))
                for k in range(len(seg)):
                    rows.append(np.concatenate([seg[k], [t]]))
                    ids.append(wid[k])
    finally:
        a.close()
    rows, ids = np.array(rows, np.float32), np.array(ids, np.int32)
    rays = np.ascontiguousarray(rows[:, [0, 1, 2, 3, 4, 5, 10]])
    wi, wt, wrec, wmat, wside, wins = AU.merged(pl, rays, records=True)
    print(f"{len(rows)} segments, {wins.sum()} won by an affine placement, {len(set(times))} distinct times")
    # (that the test is about affine placements: they win a tenth of the segments at least, at times that differ)
    assert wins.sum() >= 0.1 * len(rows) and len(set(times)) >= 100
    assert np.array_equal(ids[:, 0], wi), np.nonzero(ids[:, 0] != wi)[0][:5]
    hit = wi >= 0
    assert np.array_equal(bits(rows[hit, 6]), bits(wt[hit]))
    assert np.array_equal(bits(rows[hit, 7:10]), bits(wrec[hit, 3:6])), np.nonzero((bits(rows[:, 7:10]) != bits(wrec[:, 3:6])).any(axis=1) & hit)[0][:5]
    # the chain: a segment that follows another within a sample starts at that one's hit point
    first = np.zeros(len(rows), bool)
    first[starts] = True
    nxt = np.nonzero(~first)[0]
    assert hit[nxt - 1].all() and np.array_equal(bits(rows[nxt, :3]), bits(wrec[nxt - 1, :3]))


# ---- 12. images, kernel shapes --------------------------------------------------------------
W12, H12, SPP12 = 96, 64, 8
_REF12 = {}


def _reference12(pl):
    if "img" not in _REF12:
        a = _ctx(pl.scene)
        try:
            _REF12["img"] = a.render(_cam(0.0, 1.0, W12, H12), W12, H12, SPP12, 50, SEED)
            _REF12["segs"] = a.last_segments()
            k, st = a.last_kernel(), a.last_staging()
            assert k["persistent"] == 1 and k["grid"] == 0 and st == ALL_LDS, (k, st)
        finally:
            a.close()
        assert np.isfinite(_REF12["img"]).all() and _REF12["img"].std() > 0
    return _REF12["img"], _REF12["segs"]


@pytest.mark.parametrize("shape", ["one-shot", "persistent chunked", "one-shot chunked"])
def test_images_equal_across_kernel_shapes(shape, scene_a, monkeypatch):
    want, segs = _reference12(scene_a)
    monkeypatch.setenv("RTMI_NW_PERSIST", "0" if shape.startswith("one-shot") else "1")
    chunk = 3 if shape.endswith("chunked") else SPP12
    monkeypatch.setenv("RTMI_NW_CHUNK", str(chunk))
    a = _ctx(scene_a.scene)
    try:
        got = a.render(_cam(0.0, 1.0, W12, H12), W12, H12, SPP12, 50, SEED)
        k, st = a.last_kernel(), a.last_staging()
        assert k["persistent"] == int(not shape.startswith("one-shot")) and k["chunk"] == chunk and st == ALL_LDS, (k, st)
        assert a.last_segments() == segs
        assert np.array_equal(got, want)
    finally:
        a.close()


def test_image_row_strips_equal_the_frame(scene_a):
    import torch

    want, _ = _reference12(scene_a)
    a = _ctx(scene_a.scene)
    try:
        strip = torch.full((22, W12, 3), -1.0, dtype=torch.float32, device="cuda")
        st = torch.cuda.Stream()
        a.render_rows(_cam(0.0, 1.0, W12, H12), W12, H12, SPP12, 50, SEED, 1, 3, 22, strip.data_ptr(), st.cuda_stream)
        st.synchronize()
        img = strip.cpu().numpy()
    finally:
        a.close()
    assert np.array_equal(img[:21], want[1::3]) and (img[21] == 0).all()


def test_images_with_the_top_level_in_global_memory(monkeypatch):
    """The staging combinations of the one-shot kernel against the persistent
    one: scene A among 60 x 60 small spheres (nothing staged) and 25 x 25 (nodes
    staged, objects not)."""
    W, H = 48, 32
    for side, staging in ((60, {"nodes_lds": False, "objects_lds": False}), (25, {"nodes_lds": True, "objects_lds": False})):
        pl = _crowded(None, side)
        monkeypatch.setenv("RTMI_NW_PERSIST", "1")
        b = _ctx(pl.scene)
        monkeypatch.setenv("RTMI_NW_PERSIST", "0")
        a = _ctx(pl.scene)
        try:
            cam = _cam(0.0, 1.0, W, H)
            got, want = a.render(cam, W, H, 4, 20, SEED), b.render(cam, W, H, 4, 20, SEED)
            assert a.last_staging() == staging and a.last_kernel()["persistent"] == 0, (side, a.last_staging())
            assert (b.last_kernel()["persistent"], b.last_staging()) != (0, staging), (side, b.last_kernel(), b.last_staging())  # another shape
            assert a.last_segments() == b.last_segments() and np.array_equal(got, want) and want.std() > 0, side
        finally:
            a.close()
            b.close()


# ---- 13. frozen motion ------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0.0, THIRD, 1.0])
def test_frozen_motion_equals_the_hand_built_scene(T, scene_a):
    """Scene A at shutter [T, T] against the scene whose moving placements are
    static at off(T) — the moving affine placement a static affine one, so both
    sides run TRI = 5: hits, records and a whole image, bit for bit."""
    pl, fz = scene_a, AU.scene_a(T=T)
    assert fz.scene.motion_stats() == (0, 5) and fz.scene.affine_stats() == (3, 2)
    rays = AU.a_rays(pl, 20_000, 17, grazing=6_000)
    rays[:, 6] = np.float32(T)
    a, b = _ctx(pl.scene), _ctx(fz.scene)
    try:
        gi, gt, gf = a.debug_hits(rays)
        fi, ft, ff = b.debug_hits(rays)
        assert np.array_equal(gi, fi) and np.array_equal(bits(gt), bits(ft)) and np.array_equal(gf, ff)
        place = U.placement_of(gi, pl.first, pl.n_tri)
        assert (place == 3).mean() > 0.03 and (place == 4).mean() > 0.005
        _, _, grec, gmat = a.debug_records(rays)
        _, _, frec, fmat = b.debug_records(rays)
        assert np.array_equal(bits(grec), bits(frec)) and np.array_equal(gmat, fmat)
        cam = _cam(T, T, W12, H12)
        got, want = a.render(cam, W12, H12, SPP12, 50, SEED), b.render(cam, W12, H12, SPP12, 50, SEED)
        assert a.last_segments() == b.last_segments() and np.array_equal(got, want) and want.std() > 0
    finally:
        a.close()
        b.close()


# ---- 14. the statistical tie to the oracle's world ----------------------------------------------
def _baked_scene(pl):
    """A scene built object by object from pl's flat view at time 0 and its
    attribute records: the affine placements' triangles baked, the classical
    ones expanded — no shared mesh, so the TRI = 2 kernels render it."""
    fl, fa = pl.scene.flat(), pl.scene.flat_attr()
    obj, inst = M.flat_arrays(fl)
    s = nw.Scene()
    AU.a_mesh(s, 0)  # the materials in scene A's order: the image-textured lambertian ...
    grey = s.lambertian(s.solid(0.6, 0.5, 0.4))
    mats = [0, grey, s.metal(s.solid(0.7, 0.6, 0.5), 0.0), s.dielectric(1.5), s.lambertian(s.solid(0.9, 0.2, 0.2)),
            s.metal(s.solid(0.8, 0.7, 0.3), 0.1)]
    kind, mat, ins = obj[:, 12].view(np.int32), obj[:, 13].view(np.int32), obj[:, 14].view(np.int32)
    assert set(mat.tolist()) <= set(mats)
    tri = np.nonzero(kind == 7)[0]
    assert len(tri) == 5 * AU.A_TRIS
    for p in range(5):  # one mesh per placement: its triangles with their own corners, normals and uvs
        rows = tri[p * AU.A_TRIS:(p + 1) * AU.A_TRIS]
        at = fa["attr"][fa["attr_of_obj"][rows]]
        v = obj[rows, :9].reshape(-1, 3).astype(np.float64)
        faces = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
        smooth = bool(at[0, 15:].view(np.int32)[0] & 1)
        h = s.mesh(v, faces, normals=at[:, :9].reshape(-1, 3).astype(np.float64) if smooth else None,
                   uvs=at[:, 9:15].reshape(-1, 2).astype(np.float64), smooth=smooth, mat=int(mat[rows[0]]))
        i0 = int(ins[rows[0]])
        assert (ins[rows] == i0).all() and (i0 < 0) == (p in pl.affine)
        if i0 >= 0:  # a classical placement's Inst row: cos, sin, off
            h = s.translate(s.rotate_y(h, math.degrees(math.atan2(inst[i0, 1], inst[i0, 0]))), inst[i0, 2:5].astype(np.float64))
        s.add(h)
    for k in np.nonzero(kind != 7)[0]:
        if kind[k] == 0:
            s.add(s.sphere(obj[k, :3].astype(np.float64), float(obj[k, 3]), int(mat[k])))
        else:
            assert kind[k] == 5
            s.add(s.box(obj[k, :3].astype(np.float64), obj[k, 4:7].astype(np.float64), int(mat[k])))
    s.set_background(*[float(x) for x in fl["background"]])
    return s


def test_image_means_match_the_baked_flat_view(scene_a):
    """200 x 200 x 256 at shutter [0, 0]: the per-channel means of the whole
    image and of its four quadrants lie within 5 standard errors of a render of
    the baked flat view (TRI = 2), the standard error being the spread of the
    baked build's own means over 8 seeds, SEED .. SEED + 7; the affine scene is
    rendered at the next one, SEED + 8.
    Why not SEED + 100, as test_cornell_walls_as_triangle_pairs_match_the_
    rectangles takes it: at that seed the baked build's OWN render misses the
    bound against its 8 runs (largest |z| 5.47, blue channel of the fourth
    quadrant; the affine scene's 5.64 in the same cell), so that seed says
    nothing about the affine kernels — a "standard error" from 8 runs has 7
    degrees of freedom and 15 correlated cells are read against it.  Measured
    largest |z|, baked build / affine scene: SEED + 8: 1.59 / 1.91, SEED + 101:
    2.25 / 2.44, SEED + 102: 2.07 / 2.48.  With the SAME seed (200 x 200 x 64)
    the two scenes give the same image float for float at depths 1, 2 and 3 and
    differ in 0.0001 of the pixels, by 4e-7 of the mean, at depth 50
    (profiles/affine/README.md)."""
    W = H = 200
    spp = 256
    cam = _cam(0.0, 0.0, W, H)
    baked = _baked_scene(scene_a)

    def means(img):
        q = [img, img[:H // 2, :W // 2], img[:H // 2, W // 2:], img[H // 2:, :W // 2], img[H // 2:, W // 2:]]
        return np.array([x.mean(axis=(0, 1)) / spp for x in q])

    b = _ctx(baked, 2)
    try:
        runs = np.array([means(b.render(cam, W, H, spp, 50, SEED + k)) for k in range(8)])
    finally:
        b.close()
    a = _ctx(scene_a.scene)
    try:
        got = means(a.render(cam, W, H, spp, 50, SEED + 8))
    finally:
        a.close()
    mean, se = runs.mean(axis=0), runs.std(axis=0, ddof=1)
    z = (got - mean) / se
    print(f"baked means {mean[0]} se {se[0]}; affine {got[0]}; z whole {z[0]}, quadrants {z[1:].tolist()}")
    record_parity_stats("nw_affine_baked", {"baked_mean": mean.tolist(), "baked_se": se.tolist(), "affine_mean": got.tolist(),
                                            "z": z.tolist(), "threshold": "|z| <= 5 for the whole image and each quadrant"})
    assert (np.abs(z) <= 5).all(), z


# ---- 15. watertight on the device ----------------------------------------------------------------
def test_device_is_watertight_under_a_sheared_placement():
    v, f = M.icosphere(2)
    m = AU.shear(0.5, (2.0, 0.5, 1.3), (0.7, -0.4, 0.2))
    pl = AU.placed(lambda s: s.mesh(v, f, mat=s.lambertian(s.solid(0.5, 0.5, 0.5))), [[("transform", m)]], 320)
    rays = AU.watertight_rays(m, v, f)
    wi, wt, _, _ = AU.affine_closest(pl, rays)
    a = _ctx(pl.scene)
    try:
        gi, gt, gf = a.debug_hits(rays)
    finally:
        a.close()
    assert (gi >= 0).all() and np.array_equal(gi, wi) and np.array_equal(bits(gt), bits(wt))


# ---- 16. the CLI ----------------------------------------------------------------------------------
def test_cli_obj_tumble_matches_library(tmp_path):
    exe = os.path.join(os.path.dirname(nw.__file__), "bin", "rtmi_nw_render")
    path = tmp_path / "cube.obj"
    path.write_text(M.cube_obj("a//n", quads=True))
    W, H, spp = 24, 16, 4
    out = tmp_path / "tumbled.ppm"
    subprocess.run([exe, "--obj", str(path), "--obj-copies", "2", "--obj-tumble", "--width", str(W), "--height", str(H), "--spp", str(spp),
                    "--out", str(out)], check=True, capture_output=True, timeout=120)
    tok = out.read_text().split()
    assert tok[:4] == ["P3", str(W), str(H), "255"]
    got = np.array(tok[4:], np.int64).reshape(H, W, 3)
    s, cam, n = nw.obj_stage(path, aspect=W / H, copies=2, tumble=True)
    assert n == 12 and s.affine_stats() == (4, 0)
    r = _ctx(s)
    try:
        sums = r.render(cam, W, H, spp, 50, SEED)
    finally:
        r.close()
    mean = (sums / np.float32(spp)).astype(np.float32)
    want = np.floor(255.99 * np.sqrt(mean).astype(np.float32).astype(np.float64)).astype(np.int64)[::-1]
    assert np.array_equal(got, want) and len(np.unique(got.reshape(-1, 3), axis=0)) > 20
    plain, _, _ = nw.obj_stage(path, aspect=W / H, copies=2)
    r = _ctx(plain, 3)
    try:
        assert not np.array_equal(r.render(cam, W, H, spp, 50, SEED), sums)
    finally:
        r.close()
