"""Moving placements (Scene.move) on the GPU: the TRI = 4 kernels.  A moving
scene seen at one instant T is a static shared-mesh scene, so everything is
checked bit for bit against (a) the oracle on Scene.flat(time=T) and (b) a
second context holding the hand-built frozen scene, rendered by the TRI = 3
kernels: closest hits, hit records, whole images in every kernel shape, every
segment of open-shutter paths — and, with the shutter open, invariants of a
moving light.  Scenes and the numpy restatement of off(T): tests/nw_motion_util.py."""
import math
import os
import subprocess

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd.nextweek as nw
import nw_instance_util as U
import nw_mesh_util as M
import nw_motion_util as V
import nw_smooth_util as SU
import oracle_py as O

pytestmark = pytest.mark.gpu
SEED = 1984
THIRD = float(np.float32(1) / np.float32(3))
ALL_LDS = {"nodes_lds": True, "objects_lds": True}  # the top level; pools and bottom levels stay in global memory


def _ctx(scene, tri):
    r = nw.NwRenderer(scene)
    assert r.scene_tri() == tri and r.accel_info()["accel"] == "bvh", (r.scene_tri(), tri)
    return r


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def c_ends():
    return V.m_c_ends()


# ---- 7. frozen hits -------------------------------------------------------------
def test_hits_equal_the_frozen_scenes(c_ends):
    """Oracle's shares of the rays won by the second / third placement, per time group:
    0: .097 .060   1: .093 .058   0.5: .092 .065   1/3: .097 .064   0.1: .086 .064   0.25: .100 .064   0.75: .096 .057
    nextafter(1, 0): .095 .055"""
    moving = V.scene_m("moving")
    rays = SU.hit_rays(moving.flat(time=0.5), 40_000, 43)
    times = np.array(V.RAY_TIMES, np.float32)
    rays[:, 6] = times[np.arange(len(rays)) % 8]
    a = _ctx(moving, 4)
    try:
        gi, gt, gf = a.debug_hits(rays)
    finally:
        a.close()
    for g, T in enumerate(V.RAY_TIMES):
        sel = np.arange(len(rays)) % 8 == g
        flat = moving.flat(time=T)
        wi, wt, wf = O.nw_hits(flat, rays[sel])
        pl = U.placement_of(wi, [0, V.M_TRIS, 2 * V.M_TRIS], V.M_TRIS)
        print(f"T {T}: shares {(pl == 1).mean():.3f} {(pl == 2).mean():.3f}")
        assert (pl == 1).mean() >= 0.05 and (pl == 2).mean() >= 0.05, (T, (pl == 1).mean(), (pl == 2).mean())
        b = _ctx(V.scene_m("frozen", T, c_ends), 3)
        try:
            fi, ft, ff = b.debug_hits(rays[sel])
        finally:
            b.close()
        for what, x, y, z in (("index", gi[sel], wi, fi), ("t", _bits(gt[sel]), _bits(wt), _bits(ft)), ("face", gf[sel], wf, ff)):
            assert np.array_equal(x, y), (T, what, "oracle", np.nonzero(x != y)[0][:5])
            assert np.array_equal(x, z), (T, what, "frozen TRI = 3", np.nonzero(x != z)[0][:5])


# ---- 8. frozen records ----------------------------------------------------------
@pytest.mark.parametrize("T", [0.0, THIRD, 1.0])
def test_records_equal_the_frozen_scene(T):
    v, f = M.icosphere(2)
    local = np.concatenate([M.signed_zero_rays(np.random.default_rng(5), 10_000, np.array(M.CENTRE) - 2.6, np.array(M.CENTRE) + 2.6),
                            SU.grazing_rays(v, f, 10_000)])
    rays = V.to_world(local, V.S_ROT, V.s_off(T))
    rays[:, 6] = np.float32(T)
    moving = V.scene_s("moving")
    wi, wt, wrec, wmat = O.nw_records(moving.flat(time=T), rays, flat_attr=moving.flat_attr())
    on_mesh = (wi >= 0) & (wi < V.M_TRIS)
    print(f"T {T}: on the mesh {on_mesh.mean():.3f}, grazing {on_mesh[10_000:].mean():.3f}")
    assert on_mesh.mean() > 0.3 and on_mesh[10_000:].mean() > 0.5, (on_mesh.mean(), on_mesh[10_000:].mean())
    assert (wrec[on_mesh][:, 6:8] != 0).any()  # the texture reads u, v
    a, b = _ctx(moving, 4), _ctx(V.scene_s("frozen", T), 3)
    try:
        gi, gt, grec, gmat = a.debug_records(rays)
        fi, ft, frec, fmat = b.debug_records(rays)
    finally:
        a.close()
        b.close()
    for who, (xi, xt, xrec, xmat) in (("oracle", (wi, wt, wrec, wmat)), ("frozen TRI = 3", (fi, ft, frec, fmat))):
        assert np.array_equal(gi, xi) and np.array_equal(_bits(gt), _bits(xt)) and np.array_equal(gmat, xmat), who
        bad = np.nonzero((_bits(grec) != _bits(xrec)).any(axis=1))[0]
        assert bad.size == 0, (who, bad.size, bad[:5], grec[bad[:3]], xrec[bad[:3]])


# ---- 9. frozen images -----------------------------------------------------------
W9, H9, SPP9, DEPTH9 = 96, 64, 8, 50
CAM_M = dict(lookfrom=(2.0, 4.5, 15.0), lookat=(0.4, 0.4, 1.4), vfov=40)
CAM_F = dict(lookfrom=(15.0, 7.0, 17.0), lookat=(4.0, 0.0, 4.0), vfov=35)
_REF9 = {}


def _cam9(which, T0, T1, W=W9, H=H9):
    c = CAM_M if which == "M" else CAM_F
    return nw.camera(c["lookfrom"], c["lookat"], (0, 1, 0), c["vfov"], W / H, 0.0, 10.0, T0, T1)


def _scene9(which, mode, T, c_ends):
    return V.scene_m(mode, T, c_ends) if which == "M" else V.scene_f(mode, T)


def _reference9(which, T, c_ends):
    """(oracle image of flat(time=T), its segments) — after the frozen TRI = 3
    render (persistent kernel) was found equal to it; once per scene and T."""
    if (which, T) not in _REF9:
        cam = _cam9(which, T, T)
        moving = _scene9(which, "moving", T, c_ends)
        want, segs = O.nw_render(moving.flat(time=T), cam, W9, H9, SPP9, DEPTH9, SEED)
        assert np.isfinite(want).all() and want.std() > 0
        b = _ctx(_scene9(which, "frozen", T, c_ends), 3)
        try:
            img = b.render(cam, W9, H9, SPP9, DEPTH9, SEED)
            assert b.last_segments() == segs and np.array_equal(img, want), (which, T)
        finally:
            b.close()
        _REF9[(which, T)] = (want, segs)
    return _REF9[(which, T)]


@pytest.mark.parametrize("shape", ["persistent", "one-shot", "persistent chunked", "one-shot chunked"])
@pytest.mark.parametrize("T", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("which", ["M", "F"])
def test_images_equal_the_frozen_scene(which, T, shape, c_ends, monkeypatch):
    want, segs = _reference9(which, T, c_ends)
    monkeypatch.setenv("RTMI_NW_PERSIST", "0" if shape.startswith("one-shot") else "1")  # read when the context is created
    chunk = 3 if shape.endswith("chunked") else SPP9  # 8 samples in three work items per tile, or in one
    monkeypatch.setenv("RTMI_NW_CHUNK", str(chunk))
    a = _ctx(_scene9(which, "moving", T, c_ends), 4)
    try:
        got = a.render(_cam9(which, T, T), W9, H9, SPP9, DEPTH9, SEED)
        k, st = a.last_kernel(), a.last_staging()
        assert k["persistent"] == int(not shape.startswith("one-shot")) and k["grid"] == 0 and st == ALL_LDS, (k, st)
        assert k["chunk"] == chunk, k
        assert a.last_segments() == segs
        bad = np.nonzero((got != want).any(axis=2))
        assert np.array_equal(got, want), f"{len(bad[0])} pixels differ, first (row, col) {list(zip(*bad))[:5]}"
    finally:
        a.close()


@pytest.mark.parametrize("which", ["M", "F"])
def test_image_row_strips_equal_the_frozen_scene(which, c_ends):
    import torch

    T = 0.5
    want, _ = _reference9(which, T, c_ends)
    a = _ctx(_scene9(which, "moving", T, c_ends), 4)
    try:
        strip = torch.full((22, W9, 3), -1.0, dtype=torch.float32, device="cuda")
        st = torch.cuda.Stream()
        a.render_rows(_cam9(which, T, T), W9, H9, SPP9, DEPTH9, SEED, 1, 3, 22, strip.data_ptr(), st.cuda_stream)  # rows 1, 4, ..., 61; one past H
        st.synchronize()
        img = strip.cpu().numpy()
        assert a.last_kernel()["persistent"] == 1 and a.last_staging() == ALL_LDS
    finally:
        a.close()
    assert np.array_equal(img[:21], want[1::3]) and (img[21] == 0).all()


def test_images_with_the_top_level_in_global_memory(monkeypatch):
    """The other staging combinations of the one-shot kernel: scene M's
    placements among 60 x 60 small spheres — top-level nodes too many for a
    block's LDS budget — and among 25 x 25 — nodes staged, objects not.  The
    frozen TRI = 3 render is the reference."""
    def build(mode, side, T):
        s = V.scene_m(mode, T, V.m_c_ends())
        m = s.lambertian(s.solid(0.3, 0.6, 0.8))
        for i in range(side):
            for k in range(side):
                s.add(s.sphere((-6 + 12 * i / (side - 1), -3.0 + 0.3 * ((i + k) % 3), -5 + 12 * k / (side - 1)), 0.12, m))
        return s

    monkeypatch.setenv("RTMI_NW_PERSIST", "0")
    T, W, H = 0.25, 48, 32
    for side, staging in ((60, {"nodes_lds": False, "objects_lds": False}), (25, {"nodes_lds": True, "objects_lds": False})):
        a, b = _ctx(build("moving", side, T), 4), _ctx(build("frozen", side, T), 3)
        try:
            cam = _cam9("M", T, T, W, H)
            got, want = a.render(cam, W, H, 4, 20, SEED), b.render(cam, W, H, 4, 20, SEED)
            assert a.last_staging() == staging == b.last_staging() and a.last_kernel()["persistent"] == 0, (side, a.last_staging())
            assert a.last_segments() == b.last_segments() and np.array_equal(got, want), side
        finally:
            a.close()
            b.close()


# ---- 10. open shutter, every segment ----------------------------------------------
def test_open_shutter_segments_equal_the_oracle_at_their_time():
    """200 (pixel, sample) pairs: the traced sample's time t lies in [0, 1] and
    differs between samples; the whole path — every segment's ray, t, winner,
    normal and face — is the oracle's on flat(time=t) with the shutter [t, t]
    (the same draws, the same time).  The pairs are picked from the oracle
    side: of a fixed random stream over the image, the first 100 whose path in
    the frame frozen at 0.5 touches a moving placement and the first 100 whose
    path does not; the condition is then counted at the samples' own times."""
    W, H = 48, 32
    moving = V.scene_m("moving")
    g = np.random.default_rng(21)
    mid, picks = moving.flat(time=0.5), {True: [], False: []}
    while min(len(picks[True]), len(picks[False])) < 100:
        i, j, smp = int(g.integers(0, W)), int(g.integers(0, H)), int(g.integers(0, 16))
        _, wids = O.nw_trace(mid, _cam9("M", 0.5, 0.5, W, H), W, H, 20, SEED, i, j, smp)
        on = bool(((wids[:, 0] >= V.M_TRIS) & (wids[:, 0] < 3 * V.M_TRIS)).any())
        if len(picks[on]) < 100 and (i, j, smp) not in picks[on]:
            picks[on].append((i, j, smp))
    a = _ctx(moving, 4)
    times, touched, nseg = [], 0, 0
    try:
        for i, j, smp in picks[True] + picks[False]:
            seg, ids, t = a.debug_trace(_cam9("M", 0.0, 1.0, W, H), W, H, i, j, smp, max_depth=20, seed=SEED, with_time=True)
            assert 0.0 <= t <= 1.0
            times.append(float(t))
            wseg, wids = O.nw_trace(moving.flat(time=float(t)), _cam9("M", float(t), float(t), W, H), W, H, 20, SEED, i, j, smp)
            assert np.array_equal(ids, wids) and np.array_equal(_bits(seg), _bits(wseg)), (i, j, smp, t)
            touched += bool(((wids[:, 0] >= V.M_TRIS) & (wids[:, 0] < 3 * V.M_TRIS)).any())
            nseg += len(wseg)
    finally:
        a.close()
    print(f"{touched} of 200 paths touch a moving placement, {nseg} segments")
    assert touched >= 30 and len(set(times)) >= 190, (touched, len(set(times)))


# ---- 11. open shutter, image invariants --------------------------------------------
def test_open_shutter_light_invariants():
    W, H, spp = 64, 64, 32
    full = np.array([4, 4, 3], np.float32) * np.float32(spp)
    # from the oracle alone: the pixels whose lit state differs among 17 frozen frames
    lit = []
    for k in range(17):
        fr, _ = O.nw_render(V.scene_l("moving").flat(time=k / 16), V.camera_l(W, H, k / 16, k / 16), W, H, spp, 50, SEED)
        lit.append((fr > 0).any(axis=2))
    lit = np.array(lit)
    changing = lit.any(axis=0) & ~lit.all(axis=0)
    print(f"pixels whose lit state changes {changing.mean():.3f}")
    assert changing.mean() >= 0.05
    a = _ctx(V.scene_l("moving"), 4)
    try:
        got = a.render(V.camera_l(W, H), W, H, spp, 50, SEED)
        assert a.last_kernel()["persistent"] == 1 and a.last_staging() == ALL_LDS
    finally:
        a.close()
    ends = []
    for T in (0.0, 1.0):
        b = _ctx(V.scene_l("frozen", T), 3)
        try:
            ends.append(b.render(V.camera_l(W, H), W, H, spp, 50, SEED))
        finally:
            b.close()
    # (a) lit in every sample at both ends -> in every sample at every time between (the mesh is convex)
    both = (ends[0] == full).all(axis=2) & (ends[1] == full).all(axis=2)
    assert both.sum() > 20 and (got[both] == full).all(), both.sum()
    # (b) blur: pixels strictly between nothing and the full value
    partial = (got[..., 0] > 0) & (got[..., 0] < full[0])
    print(f"fully lit at both ends {both.sum()} pixels, partially lit {partial.mean():.3f}")
    assert partial.mean() >= 0.05
    # (c) offset0 == offset1: the static image
    c, d = _ctx(V.scene_l("moving", l1=V.L0), 4), _ctx(V.scene_l("static"), 3)
    try:
        x, y = c.render(V.camera_l(W, H), W, H, spp, 50, SEED), d.render(V.camera_l(W, H), W, H, spp, 50, SEED)
        assert c.last_segments() == d.last_segments() and np.array_equal(x, y) and x.std() > 0
    finally:
        c.close()
        d.close()


# ---- 12. mixed materials -------------------------------------------------------------
@pytest.mark.parametrize("persist", ["1", "0"])
def test_mixed_materials_equal_the_frozen_scene(persist, monkeypatch):
    W, H, T = 64, 48, THIRD
    cam = nw.camera((7, 3.0, 9), (0.3, 0.2, 0.9), (0, 1, 0), 35, W / H, 0.0, 10.0, T, T)
    monkeypatch.setenv("RTMI_NW_PERSIST", persist)
    a, b = _ctx(V.scene_x("moving"), 4), _ctx(V.scene_x("frozen", T), 3)
    try:
        got, want = a.render(cam, W, H, 16, 10, SEED), b.render(cam, W, H, 16, 10, SEED)
        assert a.last_kernel()["persistent"] == int(persist) == b.last_kernel()["persistent"] and a.last_staging() == ALL_LDS
        assert a.last_segments() == b.last_segments()
        assert np.array_equal(got, want) and np.isfinite(want).all() and want.std() > 0
    finally:
        a.close()
        b.close()


# ---- 13. the CLI -----------------------------------------------------------------------
def _run_cli(exe, path, out, extra, W=48, H=32, spp=4):
    subprocess.run([exe, "--obj", str(path), "--width", str(W), "--height", str(H), "--spp", str(spp), "--out", str(out), *extra],
                   check=True, capture_output=True, timeout=120)
    tok = out.read_text().split()
    assert tok[:4] == ["P3", str(W), str(H), "255"]
    return np.array(tok[4:], np.int64).reshape(H, W, 3)


def _ppm_of(sums, spp):
    mean = (sums / np.float32(spp)).astype(np.float32)
    return np.floor(255.99 * np.sqrt(mean).astype(np.float32).astype(np.float64)).astype(np.int64)[::-1]


def test_cli_obj_move_matches_the_raised_copies(tmp_path):
    exe = os.path.join(os.path.dirname(nw.__file__), "bin", "rtmi_nw_render")
    path = tmp_path / "cube.obj"
    path.write_text(M.cube_obj("a//n", quads=True, scale=2.0, offset=(-1.0, 0.0, -1.0)))  # the stage's box: staged as it is
    W, H, spp, copies = 48, 32, 4, 2
    got = _run_cli(exe, path, tmp_path / "moved.ppm", ["--obj-copies", "2", "--obj-move", "0,0.4,0", "--shutter", "0.5,0.5"])
    # the same stage built here, the copies raised by off(0.5) = 0 + 0.5 * (float(0.4) - 0)
    _, cam, _ = nw.obj_stage(path, aspect=W / H, copies=copies)
    cam.time0 = cam.time1 = 0.5
    raise_y = float(np.float32(0.5) * np.float32(0.4))
    s = nw.Scene()
    mesh, n = s.load_obj(path, s.lambertian(s.solid(0.7, 0.35, 0.2)))
    assert n == 12
    s.add(s.sphere((0, -1000, 0), 1000, s.lambertian(s.checker(s.solid(0.2, 0.3, 0.1), s.solid(0.9, 0.9, 0.9)))))
    h = s.shared(mesh)
    for i in range(copies):
        for k in range(copies):
            q = i * copies + k
            off = (3.0 * (i - 0.5 * (copies - 1)) + 0.4 * math.sin(1.7 * q), raise_y, 3.0 * (k - 0.5 * (copies - 1)) + 0.4 * math.cos(2.3 * q))
            s.add(s.translate(s.rotate_y(h, 37.0 * q), off))
    s.add(s.rect("xz", -1.5, 1.5, -1.5, 1.5, 5.0, s.diffuse_light(s.solid(6, 6, 6))))
    s.set_background(0.05, 0.07, 0.12)
    moving, _, _ = nw.obj_stage(path, aspect=W / H, copies=copies, move=(0, 0.4, 0))
    assert V.flats_equal(moving.flat(time=0.5), s.flat()) is None
    r = _ctx(s, 3)
    want = _ppm_of(r.render(cam, W, H, spp, 50, SEED), spp)
    r.close()
    assert np.array_equal(got, want) and len(np.unique(got.reshape(-1, 3), axis=0)) > 20
    # without --obj-move: what the command line gave before (the static copies), whatever the shutter
    still, cam0, _ = nw.obj_stage(path, aspect=W / H, copies=copies)
    r = _ctx(still, 3)
    want0 = _ppm_of(r.render(cam0, W, H, spp, 50, SEED), spp)
    r.close()
    plain = _run_cli(exe, path, tmp_path / "plain.ppm", ["--obj-copies", "2"])
    shut = _run_cli(exe, path, tmp_path / "shut.ppm", ["--obj-copies", "2", "--shutter", "0.5,0.5"])
    assert np.array_equal(plain, want0) and np.array_equal(shut, want0) and not np.array_equal(plain, got)
